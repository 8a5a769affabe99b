"""Float64 restatement of spconv's sparse 3-D convolutions and of mmdet3d's SparseEncoder for the
tests (tests/test_sparse_host.py, tests/test_gpu_sparse.py, tests/test_gpu_sparse_edges.py), on the CPU: densify the rows, run
torch.nn.functional.conv3d in double, mask.  The active mask of a strided convolution is
``conv3d(mask, ones, stride, padding) > 0``; BN uses the running statistics.  The rulebook
restatement is a coordinate -> row dictionary.  Nothing here touches the native library."""
import functools

import torch
import torch.nn.functional as F

REF_ENCODER_CFG = dict(
    type="SparseEncoder", in_channels=5, sparse_shape=[41, 1440, 1440], output_channels=128,
    order=("conv", "norm", "act"), encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
    encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, [0, 1, 1]), (0, 0)), block_type="basicblock")

# the strided forms of the reference encoder: (kernel, stride, padding)
DOWN_FORMS = {"k3s2p1": (3, 2, 1), "k3s2p011": (3, 2, (0, 1, 1)), "k311s211p0": ((3, 1, 1), (2, 1, 1), 0)}
# further forms the C entry points accept (tests/test_gpu_sparse_edges.py).  In k3s2p0, k2s2p0, k3s3p0 and k1s2p0
# some inputs of the (9, 16, 24) active set lie in no window; k3s1p1 grows the set twelvefold.
MORE_FORMS = {"k3s2p0": (3, 2, 0), "k2s2p0": (2, 2, 0), "k3s3p0": (3, 3, 0), "k3s1p1": (3, 1, 1),
              "k133s122p011": ((1, 3, 3), (1, 2, 2), (0, 1, 1)), "k3s2p2": (3, 2, 2), "k1s2p0": (1, 2, 0)}


def triple(v):
    return tuple(int(x) for x in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


@functools.lru_cache(maxsize=None)
def active_set(shape=(9, 16, 24), B=2, seed=0, n_random=220, only_sample=None):
    """Unique int32 coordinates [n, 4] (b, z, y, x) in shuffled (not ascending) row order: a seeded random
    set, one dense 3x3x3 clump, all eight corners and a run along each face.  ``only_sample``: every row in
    that sample (the other samples hold no voxel).  Do not modify the result (it is shared)."""
    D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    rows = []
    rnd = torch.stack([torch.randint(0, B, (n_random,), generator=g), torch.randint(0, D, (n_random,), generator=g),
                       torch.randint(0, H, (n_random,), generator=g), torch.randint(0, W, (n_random,), generator=g)], 1)
    rows += rnd.tolist()
    rows += [[0, 3 + dz, 5 + dy, 7 + dx] for dz in range(3) for dy in range(3) for dx in range(3)]
    rows += [[B - 1, z, y, x] for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    rows += [[0, 0, 2, x] for x in range(W)] + [[0, D - 1, y, 3] for y in range(H)]          # z faces
    rows += [[B - 1, z, 0, 4] for z in range(D)] + [[B - 1, 2, H - 1, x] for x in range(W)]  # y faces
    rows += [[0, z, 6, 0] for z in range(D)] + [[B - 1, 5, y, W - 1] for y in range(H)]      # x faces
    c = torch.tensor(rows, dtype=torch.int64)
    if only_sample is not None:
        c[:, 0] = only_sample
    c = c[(c[:, 1] < D) & (c[:, 2] < H) & (c[:, 3] < W)]   # a grid too small for the clump keeps what fits
    c = torch.unique(c, dim=0)
    c = c[torch.randperm(c.shape[0], generator=g)]
    return c.to(torch.int32).contiguous()


def lookup_table(coors):
    return {tuple(r): i for i, r in enumerate(coors.tolist())}


def out_shape(shape3, kernel, stride, padding):
    k, s, p = triple(kernel), triple(stride), triple(padding)
    return tuple((n + 2 * p[i] - k[i]) // s[i] + 1 for i, n in enumerate(shape3))


def densify(feats, coors, grid):
    """rows -> ([B, C, D, H, W] float64, mask [B, 1, D, H, W] float64)"""
    B, D, H, W = grid
    c = coors.long()
    x = torch.zeros((B, feats.shape[1], D, H, W), dtype=torch.float64)
    m = torch.zeros((B, 1, D, H, W), dtype=torch.float64)
    x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = feats.double()
    m[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = 1.0
    return x, m


def rows_of(dense, coors):
    c = coors.long()
    return dense[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


def mask_coors(mask):
    """the active sites of a mask in ascending (b, z, y, x) order, int32 [n, 4]"""
    return torch.nonzero(mask[:, 0] > 0).to(torch.int32)


def down_mask(mask, kernel, stride, padding):
    k = triple(kernel)
    return (F.conv3d(mask, torch.ones((1, 1) + k, dtype=torch.float64), stride=triple(stride),
                     padding=triple(padding)) > 0).double()


def conv_dense(x, mask, w, *, subm, stride=1, padding=0, scale=None, shift=None, residual=None, relu=True):
    """One sparse convolution on the dense form.  w (Cout, kD, kH, kW, Cin).  -> (y, out mask)"""
    wd = w.double().permute(0, 4, 1, 2, 3)
    k = tuple(w.shape[1:4])
    if subm:
        y, om = F.conv3d(x, wd, padding=tuple(v // 2 for v in k)), mask
    else:
        y, om = F.conv3d(x, wd, stride=triple(stride), padding=triple(padding)), down_mask(mask, k, stride, padding)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)
    if residual is not None:
        y = y + residual
    if relu:
        y = torch.relu(y)
    return y * om, om


def nbr_subm(coors, kernel=3):
    k = triple(kernel)
    table = lookup_table(coors)
    out = []
    for b, z, y, x in coors.tolist():
        out.append([table.get((b, z + kz - k[0] // 2, y + ky - k[1] // 2, x + kx - k[2] // 2), -1)
                    for kz in range(k[0]) for ky in range(k[1]) for kx in range(k[2])])
    return torch.tensor(out, dtype=torch.int32).reshape(len(out), k[0] * k[1] * k[2])


def nbr_down(coors, out_coors, kernel, stride, padding):
    k, s, p = triple(kernel), triple(stride), triple(padding)
    table = lookup_table(coors)
    out = []
    for b, z, y, x in out_coors.tolist():
        out.append([table.get((b, z * s[0] - p[0] + kz, y * s[1] - p[1] + ky, x * s[2] - p[2] + kx), -1)
                    for kz in range(k[0]) for ky in range(k[1]) for kx in range(k[2])])
    return torch.tensor(out, dtype=torch.int32).reshape(len(out), k[0] * k[1] * k[2])


def _taps(k):
    return [(kz, ky, kx) for kz in range(k[0]) for ky in range(k[1]) for kx in range(k[2])]


def nbr_table(coors, grid, kernel=3, out_coors=None, stride=1, padding=None):
    """nbr_subm (and, with ``out_coors``, nbr_down) without a Python loop over rows: a padded int64 table of
    row numbers, -1 elsewhere, gathered at the K shifted positions.  Equal coordinates: the lowest row."""
    B, D, H, W = grid
    k, s = triple(kernel), triple(stride)
    p = tuple(v // 2 for v in k) if padding is None else triple(padding)
    c = coors.long()
    Dp, Hp, Wp = D + 2 * p[0], H + 2 * p[1], W + 2 * p[2]
    site = ((c[:, 0] * Dp + c[:, 1] + p[0]) * Hp + c[:, 2] + p[1]) * Wp + c[:, 3] + p[2]
    table = torch.full((B * Dp * Hp * Wp,), -1, dtype=torch.int64)
    table.scatter_reduce_(0, site, torch.arange(c.shape[0]), "amin", include_self=False)
    table = table.view(B, Dp, Hp, Wp)
    q = c if out_coors is None else out_coors.long()
    b, z, y, x = q[:, 0], q[:, 1] * s[0], q[:, 2] * s[1], q[:, 3] * s[2]   # window start, in padded coordinates
    cols = [table[b, z + kz, y + ky, x + kx] for kz, ky, kx in _taps(k)]
    return torch.stack(cols, 1).to(torch.int32)


def down_coors(coors, shape, kernel, stride, padding):
    """The output coordinates of a strided convolution from the input coordinates alone (no dense tensor):
    every (c + p - kk) that is non-negative, divisible by the stride and inside out_shape; unique, ascending."""
    k, s, p = triple(kernel), triple(stride), triple(padding)
    c = coors.long()
    out = out_shape(shape, k, s, p)
    st, lim = torch.tensor(s), torch.tensor(out)
    found = []
    for kk in _taps(k):
        t = c[:, 1:] + torch.tensor(p) - torch.tensor(kk)
        o = torch.div(t, st, rounding_mode="floor")
        ok = (t >= 0).all(1) & (o * st == t).all(1) & (o < lim).all(1)
        b, o = c[ok, 0], o[ok]
        found.append(((b * out[0] + o[:, 0]) * out[1] + o[:, 1]) * out[2] + o[:, 2])   # ascending = (b, z, y, x)
    site = torch.unique(torch.cat(found))
    cols = [site // (out[0] * out[1] * out[2]), site // (out[1] * out[2]) % out[0], site // out[2] % out[1],
            site % out[2]]
    return torch.stack(cols, 1).to(torch.int32)


def rows_in_no_window(coors, out_coors, kernel, stride, padding):
    """how many input rows no output row's window holds (nbr_down names them nowhere)"""
    named = nbr_down(coors, out_coors, kernel, stride, padding)
    return coors.shape[0] - torch.unique(named[named >= 0]).numel()


def conv_rows(feats, nbr, w, scale=None, shift=None, residual=None, relu=True):
    """The same convolution evaluated only at the rows of a rulebook (no dense tensor): float64 [rows, Cout]"""
    K = nbr.shape[1]
    wk = w.double().reshape(w.shape[0], K, w.shape[-1])           # [Cout][K][Cin]
    x = torch.cat([feats.double(), torch.zeros((1, feats.shape[1]), dtype=torch.float64)], 0)
    idx = nbr.long()
    idx = torch.where(idx < 0, torch.full_like(idx, feats.shape[0]), idx)
    y = torch.zeros((nbr.shape[0], w.shape[0]), dtype=torch.float64)
    for k in range(K):
        y += x[idx[:, k]] @ wk[:, k].t()
    if scale is not None:
        y = y * scale.double() + shift.double()
    if residual is not None:
        y = y + residual.double()
    return torch.relu(y) if relu else y


def _split_bf16(t):
    t32 = t.float()
    hi = t32.bfloat16().float()
    lo = (t32 - hi).bfloat16().float()       # t32 - hi is exact in fp32
    return hi.double(), lo.double()


def conv_rows_x3(feats, nbr, w, scale=None, shift=None, residual=None, relu=True):
    """conv_rows on the kernel's three-pass arithmetic, in float64: hi = bf16(x) RNE, lo = bf16(x - hi) of both
    operands, every product lo*hi + hi*lo + hi*hi (lo*lo dropped), sums and epilogue exact."""
    K = nbr.shape[1]
    wh, wl = _split_bf16(w.reshape(w.shape[0], K, w.shape[-1]))   # [Cout][K][Cin]
    zero = torch.zeros((1, feats.shape[1]), dtype=torch.float64)
    xh, xl = (torch.cat([t, zero], 0) for t in _split_bf16(feats))
    idx = nbr.long()
    idx = torch.where(idx < 0, torch.full_like(idx, feats.shape[0]), idx)
    y = torch.zeros((nbr.shape[0], w.shape[0]), dtype=torch.float64)
    for k in range(K):
        h, l = xh[idx[:, k]], xl[idx[:, k]]
        y += l @ wh[:, k].t() + h @ wl[:, k].t() + h @ wh[:, k].t()
    if scale is not None:
        y = y * scale.double() + shift.double()
    if residual is not None:
        y = y + residual.double()
    return torch.relu(y) if relu else y


def bn_fold(bn):
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.double() * scale


def seed_encoder(enc, seed):
    """Seeded weights and BN statistics.  BN variances stay in [0.5, 2] and conv weights are
    N(0, 3 / fan_in) -- only a share of a sparse window's taps is active, so this keeps the sums near
    unit scale -- so the activations neither vanish nor blow up over the encoder's 21 convolutions
    (RMS 0.3 .. 2.5 per layer on the test's inputs)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in enc.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            if t.dim() == 5:
                fan_in = t.shape[1] * t.shape[2] * t.shape[3] * t.shape[4]
                t.copy_(torch.randn(t.shape, generator=g) * (3.0 / fan_in) ** 0.5)
            elif name.endswith("running_var"):
                t.copy_(0.5 + 1.5 * torch.rand(t.shape, generator=g))
            elif name.endswith("running_mean") or name.endswith("bias"):
                t.copy_(0.2 * torch.randn(t.shape, generator=g))
            else:   # BN weight
                t.copy_(0.8 + 0.4 * torch.rand(t.shape, generator=g))
    return enc


def encoder_dense(enc, feats, coors, B):
    """SparseEncoder.forward in float64 on the dense form -> ([B, C * D', H', W'], mask [B, 1, D', H', W'])"""
    def unit(x, m, u):
        conv, bn = u[0], u[1]
        s, b = bn_fold(bn)
        return conv_dense(x, m, conv.weight.detach(), subm=conv.subm, stride=conv.stride, padding=conv.padding,
                          scale=s, shift=b)

    x, m = densify(feats, coors, (B,) + tuple(enc.sparse_shape))
    x, m = unit(x, m, enc.conv_input)
    for stage in enc.encoder_layers:
        for blk in stage:
            if hasattr(blk, "conv1"):
                s1, b1 = bn_fold(blk.bn1)
                s2, b2 = bn_fold(blk.bn2)
                h, _ = conv_dense(x, m, blk.conv1.weight.detach(), subm=True, scale=s1, shift=b1)
                x, _ = conv_dense(h, m, blk.conv2.weight.detach(), subm=True, scale=s2, shift=b2, residual=x)
            else:
                x, m = unit(x, m, blk)
    x, m = unit(x, m, enc.conv_out)
    Bn, C, D, H, W = x.shape
    return x.reshape(Bn, C * D, H, W), m
