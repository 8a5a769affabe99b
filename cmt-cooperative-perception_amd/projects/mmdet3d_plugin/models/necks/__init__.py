from .second_fpn import SECONDFPN  # noqa: F401

__all__ = ["SECONDFPN"]
