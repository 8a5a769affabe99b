"""csrc/sparse.hip off the corridor test_gpu_sparse.py walks: the convolution on hand-made rulebooks (every NB,
column masks past the first block, the mixed vector / scalar gather, strided and misaligned operands, row
tails of the 128-row tile and the 32-row wave, untouched surroundings), device-side counts below, at and
beyond the rows, duplicate and out-of-grid coordinates, further kernel / stride / padding forms, the
two-level scan with every word populated and with more than 1024 scan blocks, and the encoder's empty
sample, empty input and repacking.

Every comparison is against float64 or exact integers of the restatement (tests/_sparse_ref.py); the one
kernel-to-kernel comparison is the bit-equality of the vector and the scalar gather on identical values.

Bounds.  (a) the project's own of test_conv_against_float64, 2^-15 sqrt(K Cin) 4 max(scale), scaled by 2^+-30
where the inputs are.  (b) against conv_rows_x3, the float64 emulation of the three-pass arithmetic: with E the
emulation's own error against float64 in the same case, the kernel must stay within 2 E + 2e-5 max(scale)
(the margin of test_gpu_train_attn_x3.py: the kernel differs from the emulation by its fp32 accumulation
only).  Neither is tuned to the kernel's output."""
import math

import pytest
import torch

import _sparse_ref as R
from test_gpu_sparse import B, ENCODER_BOUND, GRID, SHAPE, _count, _encoder, _encoder_voxels, _S

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
EPILOGUES = ((False, False), (True, True), (False, True), (True, False))   # (residual, relu)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the convolution on hand-made rulebooks ----------------------------------------------------------------

def _hand_nbr(rows, K, n_in, p_empty, g, valid=None):
    """each entry -1 with probability p_empty, else a row of ``valid`` (default: any of n_in)"""
    pick = torch.randint(0, n_in if valid is None else valid.numel(), (rows, K), generator=g)
    if valid is not None:
        pick = valid[pick]
    empty = torch.rand(rows, K, generator=g) < p_empty
    return torch.where(empty, torch.full_like(pick, -1), pick).to(torch.int32)


def _hand_case(cin, cout, K, rows, p_empty, seed, n_in=300, valid=None):
    g = torch.Generator().manual_seed(seed * 100003 + cin * 131 + cout * 7 + K)
    nbr = _hand_nbr(rows, K, n_in, p_empty, g, valid)
    x = torch.randn(n_in, cin, generator=g)
    w = torch.randn(cout, K, 1, 1, cin, generator=g)
    scale, shift = 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g)
    res = torch.randn(rows, cout, generator=g)
    return nbr, x, w, scale, shift, res


def _bound(K, cin, scale):
    return 2.0 ** -15 * math.sqrt(K * cin) * 4 * scale.max().item()


def _assert_close(got, x, nbr, w, scale, shift, res, relu, what, factor=1.0):
    """got (the kernel's rows, on the host) against conv_rows under bound (a) and, through conv_rows_x3, (b);
    ``factor``: the power of two the inputs were scaled by (shift and residual absent).  -> (err, E)"""
    want = R.conv_rows(x, nbr, w, scale, shift, res, relu)
    emu = R.conv_rows_x3(x, nbr, w, scale, shift, res, relu)
    err = (got.double() / factor - want).abs().max().item()
    E = (emu - want).abs().max().item()
    print(f"{what}: err {err:.3e} E {E:.3e}")
    bound = _bound(nbr.shape[1], x.shape[1], scale)
    assert torch.isfinite(got).all(), what
    assert err <= bound, (what, err, bound)
    assert err <= 2 * E + 2e-5 * scale.max().item(), (what, err, E)
    return err, E


def _run_epilogues(dev, parity_log, what, nbr, x, w, scale, shift, res):
    """the four residual / ReLU combinations, then the inputs at 2^-30 and 2^+30"""
    S = _S()
    cout, K, cin = w.shape[0], nbr.shape[1], x.shape[1]
    xd, nd, cnt, wp = x.to(dev), nbr.to(dev), _count(nbr.shape[0], dev), S.pack_weight(w.to(dev))
    sc, sh, rs = scale.to(dev), shift.to(dev), res.to(dev)
    worst, worst_e = 0.0, 0.0
    for with_res, relu in EPILOGUES:
        got = S.conv(xd, nd, cnt, wp, sc, sh, Cin=cin, Cout=cout, relu=relu, R=rs if with_res else None).cpu()
        err, E = _assert_close(got, x, nbr, w, scale, shift, res if with_res else None, relu,
                               f"{what} res={with_res} relu={relu}")
        worst, worst_e = max(worst, err), max(worst_e, E)
    # fp32 exponent range: a power of two on the inputs is exact in every pass (no shift, no residual)
    zero = torch.zeros(cout)
    for e in (-30, 30):
        got = S.conv(xd * 2.0 ** e, nd, cnt, wp, sc, zero.to(dev), Cin=cin, Cout=cout, relu=False).cpu()
        err, E = _assert_close(got, x, nbr, w, scale, zero, None, False, f"{what} 2^{e}", factor=2.0 ** e)
        worst, worst_e = max(worst, err), max(worst_e, E)
    parity_log.append(f"sparse conv hand-made {what}: max abs err {worst:.2e}, emulated E {worst_e:.2e} "
                      f"(bounds {_bound(K, cin, scale):.2e} and 2 E + 2e-5 max scale)")


DENSITIES = {"half": 0.5, "sparse": 63.0 / 64.0}


@pytest.mark.parametrize("density", list(DENSITIES))
@pytest.mark.parametrize("cin,cout", [(8, 48), (24, 80), (20, 96), (17, 33), (40, 65), (1, 1)])
def test_conv_channel_pairs(dev, parity_log, density, cin, cout):
    """K = 27, 300 rows: the half-wave scalar fallback under the vector gather (Cin 8, 24, 40), a ragged tail
    with KC > 1 (20, 17), the column mask in a block past the first (Cout 48, 80, 33, 65), NB = 3 (80, 96, 65)"""
    nbr, x, w, scale, shift, res = _hand_case(cin, cout, 27, 300, DENSITIES[density], seed=3)
    if density == "sparse":   # most waves skip most taps; some taps are active in exactly one wave of a tile
        active = (nbr[:256] >= 0).reshape(8, 32, 27).any(1).reshape(2, 4, 27)       # tiles 0, 1: [tile][wave][tap]
        assert (active.sum(1) == 1).any() and (~active).sum() > active.sum()
    _run_epilogues(dev, parity_log, f"{density} {cin}->{cout}", nbr, x, w, scale, shift, res)


@pytest.mark.parametrize("density", list(DENSITIES))
@pytest.mark.parametrize("K", [1, 8, 9])
def test_conv_tap_counts(dev, parity_log, density, K):
    nbr, x, w, scale, shift, res = _hand_case(16, 32, K, 300, DENSITIES[density], seed=4)
    _run_epilogues(dev, parity_log, f"{density} K={K} 16->32", nbr, x, w, scale, shift, res)


@pytest.mark.parametrize("density", list(DENSITIES))
@pytest.mark.parametrize("count", [1, 31, 32, 33, 127, 128, 129, 257])
def test_conv_row_counts(dev, parity_log, density, count):
    """32 -> 64 with ``count`` rows of count + 40: the tails of the 128-row tile and the 32-row wave.  The rows
    at and beyond the count name valid input rows (not -1) and must stay as the test wrote them."""
    S = _S()
    rows = count + 40
    nbr, x, w, scale, shift, res = _hand_case(32, 64, 27, rows, DENSITIES[density], seed=5)
    g = torch.Generator().manual_seed(count)
    nbr[count:] = torch.randint(0, 300, (40, 27), generator=g).to(torch.int32)
    assert (nbr[count:] >= 0).all()
    nbr[count - 1, 13] = (7 * count) % 300           # the last counted row has a neighbour at either density
    worst, worst_e = 0.0, 0.0
    wp, cnt = S.pack_weight(w.to(dev)), _count(count, dev)
    for with_res, relu in EPILOGUES:
        out = torch.full((rows, 64), SENTINEL, device=dev)
        got = S.conv(x.to(dev), nbr.to(dev), cnt, wp, scale.to(dev), shift.to(dev), Cin=32, Cout=64, relu=relu,
                     R=res.to(dev) if with_res else None, out=out)
        assert got.data_ptr() == out.data_ptr() and got.shape == (rows, 64)
        out = out.cpu()
        assert (out[count:] == SENTINEL).all()
        err, E = _assert_close(out[:count], x, nbr[:count], w, scale, shift, res[:count] if with_res else None, relu,
                               f"{density} count={count} res={with_res} relu={relu}")
        worst, worst_e = max(worst, err), max(worst_e, E)
    parity_log.append(f"sparse conv hand-made {density} 32->64 count {count} of {rows}: max abs err {worst:.2e}, "
                      f"emulated E {worst_e:.2e}")


@pytest.mark.parametrize("density", list(DENSITIES))
@pytest.mark.parametrize("cin,cout", [(16, 48), (24, 80)])
def test_conv_operand_layout(dev, parity_log, density, cin, cout):
    """X, out= and R as column slices of wider buffers.  X at columns [1 : 1 + Cin] of an odd-width buffer (base
    off 16 bytes, ldx % 4 != 0: the scalar gather) and at [0 : Cin] with ldx = Cin + 4 (the vector gather with
    ldx > Cin).  Outside the slices X is NaN -- also the whole of every row no nbr entry names -- and Y holds a
    sentinel: the result is finite, in bound, bit-equal to the contiguous aligned call, the sentinels intact."""
    S = _S()
    rows, n_in = 300, 340
    g = torch.Generator().manual_seed(cin)
    valid = torch.randperm(n_in, generator=g)[:200]
    nbr, x, w, scale, shift, res = _hand_case(cin, cout, 27, rows, DENSITIES[density], seed=6, n_in=n_in, valid=valid)
    named = torch.zeros(n_in, dtype=torch.bool)
    named[nbr[nbr >= 0].long()] = True
    assert 0 < named.sum() <= 200
    x_clean = torch.where(named[:, None], x, torch.zeros_like(x))
    x_nan = torch.where(named[:, None], x, torch.full_like(x, float("nan")))
    nd, cnt, wp = nbr.to(dev), _count(rows, dev), S.pack_weight(w.to(dev))
    sc, sh = scale.to(dev), shift.to(dev)
    plain = S.conv(x_clean.to(dev), nd, cnt, wp, sc, sh, Cin=cin, Cout=cout, relu=True, R=res.to(dev)).cpu()
    err, E = _assert_close(plain, x_clean, nbr, w, scale, shift, res, True, f"{density} {cin}->{cout} contiguous")
    for what, col0, width in (("scalar", 1, cin + 3), ("vector", 0, cin + 4)):
        wide = torch.full((n_in, width), float("nan"))
        wide[:, col0:col0 + cin] = x_nan
        xs = wide.to(dev)[:, col0:col0 + cin]
        assert xs.stride(0) == width and (xs.data_ptr() % 16 == 0) == (what == "vector")
        assert (width % 4 == 0) == (what == "vector")
        ywide = torch.full((rows, cout + 5), SENTINEL, device=dev)
        rwide = torch.full((rows, cout + 7), float("nan"))
        rwide[:, 3:3 + cout] = res
        got = S.conv(xs, nd, cnt, wp, sc, sh, Cin=cin, Cout=cout, relu=True, R=rwide.to(dev)[:, 3:3 + cout],
                     out=ywide[:, 2:2 + cout])
        assert got.data_ptr() == ywide[:, 2:].data_ptr() and got.stride(0) == cout + 5
        ywide = ywide.cpu()
        assert (ywide[:, :2] == SENTINEL).all() and (ywide[:, 2 + cout:] == SENTINEL).all()
        y = ywide[:, 2:2 + cout]
        _assert_close(y, x_clean, nbr, w, scale, shift, res, True, f"{density} {cin}->{cout} {what} gather, sliced")
        assert torch.equal(_bits(y), _bits(plain)), what     # both gathers feed identical MFMA operands
    parity_log.append(f"sparse conv hand-made {density} {cin}->{cout} sliced X / R / out: max abs err {err:.2e}, "
                      f"emulated E {E:.2e}, scalar and vector gather bit-equal")


# ---- 2. device-side counts ------------------------------------------------------------------------------------

FORM = "k3s2p1"
K3S2P1 = R.DOWN_FORMS[FORM]


def _down(coors_d, cnt, grid, ksp, cap):
    S = _S()
    index = S.build_index(coors_d, cnt, grid)
    oc, ocnt, nbr, _, og = S.rulebook_down(coors_d, cnt, index, grid, *ksp, cap)
    assert og == (grid[0],) + R.out_shape(grid[1:], *ksp)
    return oc.cpu(), int(ocnt.item()), nbr.cpu(), ocnt, nbr


def _subm(coors_d, cnt, grid, kernel=3):
    S = _S()
    return S.rulebook_subm(coors_d, cnt, S.build_index(coors_d, cnt, grid), grid, kernel)


def test_count_below_the_rows(dev, parity_log):
    """300 rows of which the device-side count admits 200 (the padded voxelizer output): rows 200 .. 299 are
    neighbours of earlier rows, and nothing of them may show in a rulebook, a convolution or the dense map"""
    S = _S()
    full = R.active_set(SHAPE, B)[:300]
    head = full[:200]
    ref = R.nbr_subm(head)
    assert not torch.equal(R.nbr_subm(full)[:200], ref)          # the reference itself tells the two apart
    cd, cnt = full.to(dev), _count(200, dev)
    nbr_d = _subm(cd, cnt, GRID)
    nbr = nbr_d.cpu()
    assert nbr.shape == (300, 27)
    assert torch.equal(nbr[:200], ref) and (nbr[200:] == -1).all()
    # strided
    want = R.down_coors(head, SHAPE, *K3S2P1)
    assert not torch.equal(want, R.down_coors(full, SHAPE, *K3S2P1))
    oc, m, dn, ocnt, dn_d = _down(cd, cnt, GRID, K3S2P1, 8 * 300)
    assert m == want.shape[0] and torch.equal(oc[:m], want)
    assert torch.equal(dn[:m], R.nbr_down(head, want, *K3S2P1)) and (dn[m:] == -1).all()
    # the convolution: on the submanifold rulebook, then on the strided one with the strided stage's own count
    g = torch.Generator().manual_seed(31)
    x = torch.randn(300, 32, generator=g)
    scale, shift = 0.5 + torch.rand(64, generator=g), torch.randn(64, generator=g)
    for what, nd, c, rb, K in (("subm", nbr_d, cnt, ref, 27), ("k3s2p1", dn_d, ocnt, R.nbr_down(head, want, *K3S2P1), 27)):
        w = torch.randn(64, K, 1, 1, 32, generator=g)
        out = torch.full((nd.shape[0], 64), SENTINEL, device=dev)
        S.conv(x.to(dev), nd, c, S.pack_weight(w.to(dev)), scale.to(dev), shift.to(dev), Cin=32, Cout=64, out=out)
        out = out.cpu()
        rows = rb.shape[0]
        assert (out[rows:] == SENTINEL).all()
        err, E = _assert_close(out[:rows], x, rb, w, scale, shift, None, True, f"count 200 of 300 {what}")
        parity_log.append(f"sparse conv {what} with count 200 of 300 rows: max abs err {err:.2e}, emulated E {E:.2e}")
    # densify
    dense = S.to_dense(x.to(dev), cd, cnt, GRID, 32).cpu()
    want_dense, _ = R.densify(x[:200], head, GRID)
    assert torch.equal(dense, want_dense.float().reshape(B, 32 * SHAPE[0], SHAPE[1], SHAPE[2]))
    late = full[200:].long()
    assert (dense.reshape(B, 32, *SHAPE)[late[:, 0], :, late[:, 1], late[:, 2], late[:, 3]] == 0).all()


@pytest.mark.parametrize("count", [0, -1])
def test_count_of_no_rows(dev, count):
    """0, and the -1 an overflowing strided stage hands on: all -1, no output site, no Y row, a zero map"""
    S = _S()
    coors = R.active_set(SHAPE, B)[:300]
    cd, cnt = coors.to(dev), _count(count, dev)
    nbr_d = _subm(cd, cnt, GRID)
    assert nbr_d.shape == (300, 27) and (nbr_d == -1).all()
    oc, m, dn, _, dn_d = _down(cd, cnt, GRID, K3S2P1, 600)
    assert m == 0 and (dn == -1).all()
    g = torch.Generator().manual_seed(32)
    x, w = torch.randn(300, 16, generator=g).to(dev), torch.randn(32, 3, 3, 3, 16, generator=g).to(dev)
    valid_nbr = torch.randint(0, 300, (300, 27), generator=g).to(torch.int32).to(dev)    # rows the count excludes
    for nd in (nbr_d, dn_d, valid_nbr):
        out = torch.full((nd.shape[0], 32), SENTINEL, device=dev)
        S.conv(x, nd, cnt, S.pack_weight(w), torch.ones(32, device=dev), torch.ones(32, device=dev), Cin=16, Cout=32,
               out=out)
        assert (out == SENTINEL).all()
    dense = S.to_dense(x, cd, cnt, GRID, 16)
    assert dense.shape == (B, 16 * SHAPE[0], SHAPE[1], SHAPE[2]) and (dense == 0).all()


def test_count_beyond_the_rows_clamps(dev, parity_log):
    S = _S()
    coors = R.active_set(SHAPE, B)[:300]
    cd, cnt = coors.to(dev), _count(350, dev)
    nbr_d = _subm(cd, cnt, GRID)
    ref = R.nbr_subm(coors)
    assert torch.equal(nbr_d.cpu(), ref)
    want = R.down_coors(coors, SHAPE, *K3S2P1)
    oc, m, dn, _, _ = _down(cd, cnt, GRID, K3S2P1, want.shape[0])
    assert m == want.shape[0] and torch.equal(oc, want) and torch.equal(dn, R.nbr_down(coors, want, *K3S2P1))
    g = torch.Generator().manual_seed(33)
    x, w = torch.randn(300, 16, generator=g), torch.randn(32, 27, 1, 1, 16, generator=g)
    scale, shift = 0.5 + torch.rand(32, generator=g), torch.randn(32, generator=g)
    got = S.conv(x.to(dev), nbr_d, cnt, S.pack_weight(w.to(dev)), scale.to(dev), shift.to(dev), Cin=16, Cout=32).cpu()
    assert got.shape == (300, 32)
    err, E = _assert_close(got, x, ref, w, scale, shift, None, True, "count 350 of 300")
    parity_log.append(f"sparse conv subm with count 350 of 300 rows: max abs err {err:.2e}, emulated E {E:.2e}")
    dense = S.to_dense(x.to(dev), cd, cnt, GRID, 16).cpu()
    assert torch.equal(dense, R.densify(x, coors, GRID)[0].float().reshape(B, 16 * SHAPE[0], SHAPE[1], SHAPE[2]))


# ---- 3. duplicate and out-of-grid coordinates -----------------------------------------------------------------

def test_duplicate_coordinates_resolve_to_the_first_row(dev):
    base = R.active_set(SHAPE, B)[:300]
    pick = torch.arange(7, 300, 15)[:20]
    assert pick.numel() == 20
    coors = torch.cat([base, base[pick]]).contiguous()
    cd, cnt = coors.to(dev), _count(320, dev)
    nbr = _subm(cd, cnt, GRID).cpu()
    ref = R.nbr_subm(base)
    assert (ref[:, None, :] == pick[None, :, None]).any()          # other rows do name the duplicated sites
    assert nbr.max().item() < 300                                  # never a copy: the lowest row index
    assert torch.equal(nbr[:300], ref)                             # the other entries are unchanged
    assert torch.equal(nbr[300:], ref[pick])                       # a copy sees what its original sees
    want = R.down_coors(base, SHAPE, *K3S2P1)
    oc, m, dn, _, _ = _down(cd, cnt, GRID, K3S2P1, want.shape[0])
    assert m == want.shape[0] and torch.equal(oc, want) and torch.equal(dn, R.nbr_down(base, want, *K3S2P1))


def test_out_of_grid_rows_are_ignored(dev):
    """rows with b = B, z = -1, y = H, x = -5 among the valid ones: no valid row's entry names one, and the
    rulebooks and the dense map are those of the valid rows alone, renumbered"""
    S = _S()
    valid = R.active_set(SHAPE, B)[:300]
    g = torch.Generator().manual_seed(41)
    bad = valid[torch.randperm(300, generator=g)[:24]].clone()
    bad[0::4, 0], bad[1::4, 1], bad[2::4, 2], bad[3::4, 3] = B, -1, SHAPE[1], -5
    order = torch.randperm(324, generator=g)
    coors = torch.cat([valid, bad])[order].contiguous()
    pos = torch.empty(324, dtype=torch.int64)
    pos[order] = torch.arange(324)                                 # row i of cat(valid, bad) sits at pos[i]
    vpos = pos[:300]

    def renumber(ref):
        r = ref.long()
        return torch.where(r >= 0, vpos[r.clamp(min=0)], r).to(torch.int32)

    cd, cnt = coors.to(dev), _count(324, dev)
    nbr = _subm(cd, cnt, GRID).cpu()
    assert torch.equal(nbr[vpos], renumber(R.nbr_subm(valid)))     # (the invalid rows' own nbr rows are unspecified)
    want = R.down_coors(valid, SHAPE, *K3S2P1)
    oc, m, dn, _, _ = _down(cd, cnt, GRID, K3S2P1, want.shape[0])
    assert m == want.shape[0] and torch.equal(oc, want)
    assert torch.equal(dn, renumber(R.nbr_down(valid, want, *K3S2P1)))
    x = torch.randn(324, 5, generator=g)
    dense = S.to_dense(x.to(dev), cd, cnt, GRID, 5).cpu()
    want_dense, _ = R.densify(x[vpos], valid, GRID)
    assert torch.equal(dense, want_dense.float().reshape(B, 5 * SHAPE[0], SHAPE[1], SHAPE[2]))


# ---- 4. more geometry -----------------------------------------------------------------------------------------

OUTSIDE = {"k3s2p0": 51, "k2s2p0": 39, "k3s3p0": 29, "k1s2p0": 255}     # inputs in no window, of 300


@pytest.mark.parametrize("form", list(R.MORE_FORMS))
def test_more_strided_forms(dev, parity_log, form):
    """test_rulebook_down_exact's assertions and one 32 -> 64 convolution against conv3d in float64"""
    S = _S()
    k, s, p = R.MORE_FORMS[form]
    coors = R.active_set(SHAPE, B)[:300]
    _, mask = R.densify(torch.zeros(300, 1), coors, GRID)
    want = R.mask_coors(R.down_mask(mask, k, s, p))
    m = want.shape[0]
    ref = R.nbr_down(coors, want, k, s, p)
    # the form takes sp_mark_down's rejection (an output coordinate beyond the output grid) where expected
    assert R.rows_in_no_window(coors, want, k, s, p) == OUTSIDE.get(form, 0)
    cd, cnt = coors.to(dev), _count(300, dev)
    oc, got_m, nbr, ocnt, nbr_d = _down(cd, cnt, GRID, (k, s, p), m)                # capacity exactly the true count
    assert got_m == m
    assert torch.equal(oc, want)
    assert torch.equal(nbr, ref)
    assert (nbr >= 0).any(dim=1).all()
    _, short, _, _, _ = _down(cd, cnt, GRID, (k, s, p), m - 1)
    assert short == -1
    g = torch.Generator().manual_seed(51)
    kk = R.triple(k)
    x, w = torch.randn(300, 32, generator=g), torch.randn((64,) + kk + (32,), generator=g)
    scale, shift = 0.5 + torch.rand(64, generator=g), torch.randn(64, generator=g)
    xd, _ = R.densify(x, coors, GRID)
    yd, om = R.conv_dense(xd, mask, w, subm=False, stride=s, padding=p, scale=scale, shift=shift)
    assert torch.equal(R.mask_coors(om), want)
    got = S.conv(x.to(dev), nbr_d, ocnt, S.pack_weight(w.to(dev)), scale.to(dev), shift.to(dev), Cin=32, Cout=64).cpu()
    K = kk[0] * kk[1] * kk[2]
    err = (got.double() - R.rows_of(yd, want)).abs().max().item()
    assert err <= _bound(K, 32, scale), (form, err)
    _, E = _assert_close(got, x, ref, w, scale, shift, None, True, f"{form} 32->64")
    parity_log.append(f"sparse conv {form} 32->64, {m} outputs: max abs err {err:.2e} vs conv3d, emulated E {E:.2e} "
                      f"(bound {_bound(K, 32, scale):.2e})")


@pytest.mark.parametrize("kernel", [(1, 3, 3), (3, 1, 3), 1])
def test_more_submanifold_kernels(dev, kernel):
    coors = R.active_set(SHAPE, B)[:300]
    nbr = _subm(coors.to(dev), _count(300, dev), GRID, kernel).cpu()
    ref = R.nbr_subm(coors, kernel)
    k = R.triple(kernel)
    assert nbr.shape == ref.shape == (300, k[0] * k[1] * k[2])
    assert torch.equal(nbr, ref)
    assert torch.equal(nbr[:, nbr.shape[1] // 2], torch.arange(300, dtype=torch.int32))


# ---- 5. the index scan at scale -------------------------------------------------------------------------------

def test_scan_with_every_word_populated(dev):
    """(1, 8, 200, 200): 10000 index words in 3 scan blocks, 100000 of the 320000 sites set, so every scan
    thread and every blockoff carries a count"""
    grid = (1, 8, 200, 200)
    g = torch.Generator().manual_seed(61)
    site = torch.randperm(320000, generator=g)[:100000]                         # shuffled row order
    coors = torch.stack([torch.zeros_like(site), site // 40000, site // 200 % 200, site % 200], 1).to(torch.int32)
    words = torch.zeros(10000, dtype=torch.int64).scatter_add_(0, site // 32, torch.ones_like(site))
    assert (words > 0).all()
    ref = R.nbr_table(coors, grid)
    assert 8.0 < (ref >= 0).sum().item() / 100000 < 9.0
    cd, cnt = coors.contiguous().to(dev), _count(100000, dev)
    assert torch.equal(_subm(cd, cnt, grid).cpu(), ref)
    want = R.down_coors(coors, grid[1:], *K3S2P1)
    oc, m, nbr, _, _ = _down(cd, cnt, grid, K3S2P1, want.shape[0])
    assert m == want.shape[0] and m > 39000
    assert torch.equal(oc, want)
    assert torch.equal(nbr, R.nbr_table(coors, grid, K3S2P1[0], want, K3S2P1[1], K3S2P1[2]))


def test_two_samples_on_the_full_grid(dev, parity_log):
    """(2, 41, 1440, 1440), the cooperative workload: 170 M sites, 1297 scan blocks, so sp_scan_blocks sums two
    block totals per thread; and the strided rulebook on a large grid.  Clustered sites in both samples, the
    first and last site of each, and sites either side of the boundary between the samples."""
    S = _S()
    grid = (2, 41, 1440, 1440)
    g = torch.Generator().manual_seed(71)
    centres = torch.stack([torch.randint(0, 2, (250,), generator=g), torch.randint(0, 41, (250,), generator=g),
                           torch.randint(0, 1440, (250,), generator=g), torch.randint(0, 1440, (250,), generator=g)], 1)
    near = centres.repeat_interleave(8, 0)
    near[:, 1:] += torch.randint(-1, 2, (near.shape[0], 3), generator=g)
    near[:, 1].clamp_(0, 40)
    near[:, 2:].clamp_(0, 1439)
    pinned = torch.tensor([[0, 0, 0, 0], [0, 40, 1439, 1439], [1, 0, 0, 0], [1, 40, 1439, 1439],
                           [0, 40, 1439, 1438], [0, 40, 1438, 1439], [0, 39, 1439, 1439], [1, 0, 0, 1], [1, 0, 1, 0],
                           [1, 1, 0, 0]])
    coors = torch.unique(torch.cat([centres, near, pinned]), dim=0)
    coors = coors[torch.randperm(coors.shape[0], generator=g)].to(torch.int32).contiguous()
    n = coors.shape[0]
    assert 1500 <= n <= 2300 and 0.3 * n < (coors[:, 0] == 0).sum().item() < 0.7 * n
    for pin in pinned[:4].tolist():
        assert (coors == torch.tensor(pin, dtype=torch.int32)).all(1).any()
    # the index's layout (sparse.hip: header, bits, prefix, blockoff, rank2row; rounded up to 256 bytes):
    words = (2 * 41 * 1440 * 1440 + 31) // 32
    nblocks_at_least = S.index_bytes(grid, n) // 4 - 8 - 2 * words - n - 63
    assert nblocks_at_least > 1024                                  # two block totals per scan thread
    cd, cnt = coors.to(dev), _count(n, dev)
    index = S.build_index(cd, cnt, grid)
    nbr = S.rulebook_subm(cd, cnt, index, grid)
    ref = R.nbr_subm(coors)
    assert torch.equal(nbr.cpu(), ref)
    assert (ref >= 0).sum().item() > 2 * n
    want = R.down_coors(coors, grid[1:], *K3S2P1)
    m = want.shape[0]
    oc, ocnt, dn, _, og = S.rulebook_down(cd, cnt, index, grid, *K3S2P1, m)
    assert og == (2, 21, 720, 720)
    assert int(ocnt.item()) == m and torch.equal(oc.cpu(), want)
    assert torch.equal(dn.cpu(), R.nbr_down(coors, want, *K3S2P1))
    x, w = torch.randn(n, 5, generator=g), torch.randn(16, 3, 3, 3, 5, generator=g)
    scale, shift = 0.5 + torch.rand(16, generator=g), torch.randn(16, generator=g)
    got = S.conv(x.to(dev), nbr, cnt, S.pack_weight(w.to(dev)), scale.to(dev), shift.to(dev), Cin=5, Cout=16).cpu()
    err, E = _assert_close(got, x, ref, w, scale, shift, None, True, "two samples, full grid 5->16")
    parity_log.append(f"sparse conv subm 5->16 on (2, 41, 1440, 1440), {n} rows: max abs err {err:.2e}, "
                      f"emulated E {E:.2e}")


# ---- 6. the encoder -------------------------------------------------------------------------------------------

def _encoder_error(enc_dev, enc_ref, feats, coors, dev):
    """-> (got on the host, float64 reference, mask, max abs error over the reference's max abs)"""
    want, mask = R.encoder_dense(enc_ref, feats, coors, 2)
    with torch.no_grad():
        got = enc_dev(feats.to(dev), coors.to(dev), 2).cpu()
    assert tuple(got.shape) == tuple(want.shape) == (2, 256, 4, 4) and got.dtype == torch.float32
    top = want.abs().max().item()
    assert top > 0.1
    return got, want, mask, (got.double() - want).abs().max().item() / top


def test_encoder_with_an_empty_sample(dev, parity_log):
    _, coors = _encoder_voxels()
    coors = coors.clone()
    coors[:, 0] = 1
    coors = torch.unique(coors, dim=0)
    g = torch.Generator().manual_seed(81)
    coors = coors[torch.randperm(coors.shape[0], generator=g)].contiguous()
    feats = torch.randn(coors.shape[0], 5, generator=g)
    assert coors.shape[0] >= 300 and (coors[:, 0] == 1).all()
    got, want, mask, err = _encoder_error(_encoder().to(dev), _encoder(), feats, coors, dev)
    assert mask[0].sum() == 0 and mask[1].sum() > 0 and (want[0] == 0).all()
    assert (got[0] == 0).all()                                    # exactly zero: no site of sample 0 is written
    site = (got.reshape(2, 128, 2, 4, 4) != 0).any(dim=1, keepdim=True)
    assert torch.equal(site, mask > 0)
    parity_log.append(f"SparseEncoder {coors.shape[0]} voxels, all in sample 1: max abs err / max abs {err:.2e} "
                      f"(bound {ENCODER_BOUND:.1e})")
    assert err <= ENCODER_BOUND


def test_encoder_with_no_voxel(dev):
    enc = _encoder().to(dev)
    with torch.no_grad():
        got = enc(torch.zeros(0, 5, device=dev), torch.zeros(0, 4, dtype=torch.int32, device=dev), 2)
    assert tuple(got.shape) == (2,) + enc.output_shape() == (2, 256, 4, 4)
    assert got.dtype == torch.float32 and got.device.type == "cuda" and (got == 0).all()


def test_encoder_repacks_after_an_in_place_update(dev, parity_log):
    """one forward, new weights and BN statistics written in place on the device (same storage, so only the
    version counters tell), a second forward: both match the float64 reference of the weights they ran with"""
    feats, coors = _encoder_voxels()
    enc = _encoder(11).to(dev)
    _, want1, _, err1 = _encoder_error(enc, _encoder(11), feats, coors, dev)
    assert err1 <= ENCODER_BOUND
    ptr = enc.conv_input[0].weight.data_ptr()
    R.seed_encoder(enc, 12)
    assert enc.conv_input[0].weight.data_ptr() == ptr
    fresh = _encoder(12)
    for k, v in fresh.state_dict().items():
        assert torch.equal(enc.state_dict()[k].cpu(), v), k
    assert not torch.equal(fresh.conv_input[0].weight, _encoder(11).conv_input[0].weight)
    got2, want2, _, err2 = _encoder_error(enc, fresh, feats, coors, dev)
    stale = (want1 - want2).abs().max().item() / want2.abs().max().item()
    assert stale > 100 * ENCODER_BOUND                            # stale packs would be far outside the bound
    parity_log.append(f"SparseEncoder before / after an in-place reseed: max abs err / max abs {err1:.2e} / "
                      f"{err2:.2e} (bound {ENCODER_BOUND:.1e}; the two references differ by {stale:.2e})")
    assert err2 <= ENCODER_BOUND
