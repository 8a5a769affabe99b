from .backbones import *  # noqa: F401,F403
from .dense_heads import *  # noqa: F401,F403
from .detectors import *  # noqa: F401,F403
from .middle_encoders import *  # noqa: F401,F403
from .necks import *  # noqa: F401,F403
from .utils import *  # noqa: F401,F403
from .voxel_encoders import *  # noqa: F401,F403
