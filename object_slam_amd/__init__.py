"""MI355X-native (gfx950) front-end + local-BA hot path of yangliu9527/Object_SLAM.

Thin Python view of the C ABI in include/oslam_hip.h (the product is the HIP library;
Python is harness).  Class and method names mirror the reference's C++ API.
"""
from ._lib import KP_DTYPE, OslamError  # noqa: F401
from .extractor import ORBextractor  # noqa: F401
from .matcher import BowMatcher, ORBmatcher, QUERY_DTYPE, StereoMatcher, feature_vector  # noqa: F401
from .frame import FrameOps  # noqa: F401
from .mappoint import MapPointBatch  # noqa: F401
from .optimizer import LocalBundleAdjuster, PoseOptimizer  # noqa: F401
from .vocabulary import Vocabulary  # noqa: F401
from .pnp import PnPsolver  # noqa: F401
from . import pnp  # noqa: F401
from .sim3 import Sim3Solver  # noqa: F401
from . import sim3  # noqa: F401
from .sim3_match import Sim3Matcher  # noqa: F401
from . import sim3_match  # noqa: F401
from .sim3_opt import Sim3Optimizer  # noqa: F401
from . import sim3_opt  # noqa: F401
from .sim3_project import Sim3Projector  # noqa: F401
from . import sim3_project  # noqa: F401
from .essential_graph import EssentialGraphOptimizer, essential_graph_edges  # noqa: F401
from . import essential_graph  # noqa: F401
from .keyframe_db import KeyFrameDatabase  # noqa: F401
from . import keyframe_db  # noqa: F401
from .reloc_project import RelocProjector  # noqa: F401
from . import reloc_project  # noqa: F401
from .initializer import Initializer  # noqa: F401
from . import initializer  # noqa: F401
from .search_init import InitMatcher  # noqa: F401
from . import search_init  # noqa: F401
from .object_match import ObjectMatcher  # noqa: F401
from . import object_match  # noqa: F401
from .object_map import ObjectMap  # noqa: F401
from . import object_map  # noqa: F401
from .loop_correct import LoopCorrector  # noqa: F401
from . import loop_correct  # noqa: F401
from .loop_detect import LoopDetector  # noqa: F401
from . import loop_detect  # noqa: F401
from .covisibility import CovisibilityGraph  # noqa: F401
from . import covisibility  # noqa: F401
