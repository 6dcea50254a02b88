"""Minimal `jrl` for running the reference's cppflow modules on the CPU (TEST INFRASTRUCTURE ONLY; see oracle/reference_run.py).

Only the names the reference's cppflow modules import are provided, and every one of them is this project's own code: the kinematics,
capsule distances and quaternion helpers are those of oracle/ref_torch.py.  What runs on top of them -- the residual stacking, the row
options, the search recurrence, the validity rules -- is the reference's.
"""
