"""GridMask as the reference's detectors apply it to a prepared image batch, with the mask computed on the device
(cmt_grid_mask, include/cmt_hip.h) instead of built in numpy / PIL and uploaded."""
import numpy as np
import torch.nn as nn

from ... import native_imgaug as NIA


class GridMask(nn.Module):
    """The reference's constructor arguments and ``set_prob``.  ``forward`` returns ``x`` untouched outside training
    or when ``np.random.rand() > prob``; otherwise it draws ``d = randint(2, h)``, ``st_h = randint(d)``,
    ``st_w = randint(d)`` and ``randint(rotate)`` from numpy's global stream, in that order, and masks fp32
    ``x`` [n, c, h, w] IN PLACE on the device (the reference returns a new tensor; the values are the same).
    ``rotate != 1`` (a rotated mask) and ``offset=True`` are not built."""

    def __init__(self, use_h, use_w, rotate=1, offset=False, ratio=0.5, mode=0, prob=1.):
        super().__init__()
        if rotate != 1:
            raise NotImplementedError("GridMask with rotate != 1 (a rotated mask) is not built")
        if offset:
            raise NotImplementedError("GridMask(offset=True) is not built")
        self.use_h = use_h
        self.use_w = use_w
        self.rotate = rotate
        self.offset = offset
        self.ratio = ratio
        self.mode = mode
        self.st_prob = prob
        self.prob = prob

    def set_prob(self, epoch, max_epoch):
        self.prob = self.st_prob * epoch / max_epoch

    def forward(self, x):
        conf = dict(use_h=self.use_h, use_w=self.use_w, rotate=self.rotate, offset=self.offset, ratio=self.ratio,
                    mode=self.mode, prob=self.prob)
        params = NIA.sample_grid_mask(conf, x.shape[2], np.random, training=self.training)
        if params is None:
            return x
        self.l = params["l"]
        return NIA.grid_mask_(x, params)
