You are in the lounge where all tired chatters come and rest for a short
while. Some armchairs have been placed around the room and a fire has
been stoked in the grate.
