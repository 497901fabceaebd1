from end2end_amd.functions.asg import ASGLossFunction  # noqa: F401
