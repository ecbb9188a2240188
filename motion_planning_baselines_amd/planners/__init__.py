from .prm import PRM  # noqa: F401
from .rrt_star import InfRRTStar, RRTStar  # noqa: F401
from .strrt_connect import STRRTConnect  # noqa: F401
