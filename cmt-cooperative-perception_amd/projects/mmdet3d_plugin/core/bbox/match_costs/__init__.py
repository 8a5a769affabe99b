"""Match costs of the assigner that are plain functions of device tensors."""

__all__ = ["IoU3DCost"]


class IoU3DCost:
    """-iou * weight; ``iou`` is what ``native_iou.box_iou(..., mode='3d')`` gives."""

    def __init__(self, weight):
        self.weight = weight

    def __call__(self, iou):
        return -iou * self.weight
