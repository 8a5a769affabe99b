from .second import SECOND  # noqa: F401
from .vovnet import VoVNet  # noqa: F401

__all__ = ["SECOND", "VoVNet"]
