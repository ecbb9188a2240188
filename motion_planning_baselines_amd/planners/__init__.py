from .rrt_star import InfRRTStar, RRTStar  # noqa: F401
