You are in the hallway. The large front door leads out to the drive whilst
another smaller door leads into the wizards room. A corridor leads deeper into
the mansion.
