You are on the long front gravel drive of Money Mansion. Red brick walls
and large bay windows face you along with the two pillars surrounding the
entrance to the hallway. Potted plants line the front of the building and
trees have been planted on all sides. Beyond them is a white haze where
this particular reality ends.
