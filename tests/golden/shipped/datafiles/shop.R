The shop you are in sells all manner of things but you can't buy any of it
since it is far far too expensive.
