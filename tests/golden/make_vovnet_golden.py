"""Generate the VoVNet fixtures under tests/golden/ from the reference's own class (data only):

  vovnet_keys.json     state-dict key -> shape, in order, for the four supported specs
  vovnet_v39_ref.npz   stage4 / stage5 of the reference's V-39-eSE in float64 on the seeded [2, 3, 37, 53]
                       image, every state-dict tensor seeded by key (tests/_vov_ref.seed_by_key)

The reference's models/backbones/vovnet.py is loaded by path at run time under stand-in modules for
``mmcv.runner.BaseModule`` and ``mmdet.models.builder.BACKBONES`` (neither is installed); nothing of it is
copied.  Its ``train()`` returns None, so ``.eval()`` stands on a line of its own.

    python tests/golden/make_vovnet_golden.py <reference checkout>
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _vov_ref as R  # noqa: E402

SEED, IMAGE_SEED, SHAPE = 39, 3953, (2, 3, 37, 53)


def load_reference(root):
    class BaseModule(torch.nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()
            self.init_cfg = init_cfg

    class _Registry:
        def register_module(self):
            return lambda cls: cls

    for name in ("mmcv", "mmcv.runner", "mmdet", "mmdet.models", "mmdet.models.builder"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mmcv.runner"].BaseModule = BaseModule
    sys.modules["mmdet.models.builder"].BACKBONES = _Registry()
    path = os.path.join(root, "projects", "mmdet3d_plugin", "models", "backbones", "vovnet.py")
    spec = importlib.util.spec_from_file_location("_reference_vovnet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.VoVNet


def main(root):
    VoVNet = load_reference(root)
    keys = {}
    for spec in sorted(R.SHAPE):
        m = VoVNet(spec, out_features=("stage4", "stage5"))
        keys[spec] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "vovnet_keys.json"), "w") as f:
        json.dump(keys, f, separators=(",", ":"))
    m = VoVNet("V-39-eSE", out_features=("stage4", "stage5")).double()
    m.eval()
    R.seed_by_key(m, SEED)
    x = R.seeded_image(IMAGE_SEED, SHAPE)
    with torch.no_grad():
        out = m(x.double())
    # the largest conv output on the way: the range the seeding keeps the maps in (|x| < 12 everywhere)
    peaks = []
    hooks = [mod.register_forward_hook(lambda _m, _i, o: peaks.append(o.abs().max().item()))
             for mod in m.modules() if isinstance(mod, torch.nn.Conv2d)]
    with torch.no_grad():
        m(x.double())
    for h in hooks:
        h.remove()
    peak = max(peaks)
    np.savez_compressed(os.path.join(HERE, "vovnet_v39_ref.npz"), stage4=out["stage4"].numpy(),
                        stage5=out["stage5"].numpy(), seed=np.int64(SEED), image_seed=np.int64(IMAGE_SEED),
                        shape=np.array(SHAPE, dtype=np.int64))
    print({k: (tuple(v.shape), float(v.abs().max())) for k, v in out.items()}, "largest |conv output|", peak)


if __name__ == "__main__":
    main(sys.argv[1])
