from end2end_amd.modules.asg_loss import ASGLoss, asg_loss  # noqa: F401
