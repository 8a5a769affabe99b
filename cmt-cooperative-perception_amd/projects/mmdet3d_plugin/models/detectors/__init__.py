from .cmt import CmtDetector, bbox3d2result
from .cmt_coop import CmtCoopDetector

__all__ = ["CmtDetector", "CmtCoopDetector", "bbox3d2result"]
