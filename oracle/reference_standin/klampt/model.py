"""Placeholder names of klampt.model."""

coordinates = None
trajectory = None
create = None
