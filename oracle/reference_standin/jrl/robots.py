"""jrl.robots.get_robot over this project's robot descriptions (cppflow_amd/robot_zoo.py)."""

from cppflow_amd.robot_zoo import ROBOT_SPECS
from jrl.robot import Robot


def get_robot(name: str) -> Robot:
    return Robot(ROBOT_SPECS[name]())
