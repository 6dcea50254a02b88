"""Placeholder `klampt`: the names the reference's modules import, none of which the recorded runs call (TEST INFRASTRUCTURE ONLY)."""


class RigidObjectModel:
    pass


vis = None
