from .sparse_encoder import SparseBasicBlock, SparseConv, SparseEncoder  # noqa: F401

__all__ = ["SparseEncoder", "SparseBasicBlock", "SparseConv"]
