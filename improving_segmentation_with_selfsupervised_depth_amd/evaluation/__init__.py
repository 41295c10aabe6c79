from .metrics import runningDepthScore, runningScore  # noqa: F401
