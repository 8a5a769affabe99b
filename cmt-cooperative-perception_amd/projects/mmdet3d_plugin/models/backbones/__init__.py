from .second import SECOND  # noqa: F401

__all__ = ["SECOND"]
