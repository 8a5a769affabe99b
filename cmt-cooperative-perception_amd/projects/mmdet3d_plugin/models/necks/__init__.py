from .cp_fpn import CPFPN  # noqa: F401
from .second_fpn import SECONDFPN  # noqa: F401

__all__ = ["SECONDFPN", "CPFPN"]
