You are in the corridor which leads to the back of the mansion. It is very
narrow here and the wooden panelled walls seem to press in on you. You can
wander to the hallway or into the lounge.
