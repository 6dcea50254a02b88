"""Placeholder names of klampt.math."""

so3 = None
