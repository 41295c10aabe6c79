from .metrics import AverageMeter, AverageMeterDict, runningDepthScore, runningScore  # noqa: F401
