"""cmt_lsap (csrc/assign.hip), the device-side Hungarian assignment, against
scipy.optimize.linear_sum_assignment on the same fp32 matrices, and the head's
opt-in training path through it (runtime.Options.device_assign).

Every fixture is generated here with a fixed seed.  The solver keeps its duals
and path costs in float64 like scipy, so on a matrix whose optimum is unique
the two assignments are EQUAL, not close; where an optimum is not unique (the
integer matrix) the total cost must equal scipy's exactly and the matching must
be one-to-one."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
PARITY_SHAPES = [(1, 1), (70, 5), (64, 64), (65, 64), (900, 1), (900, 37), (900, 100), (200, 200), (5, 70)]


def _l1_cost(nq, ngt, seed, noise=0.1, crowd=None):
    """|q - g| L1 over 8 channels + noise * normal, fp32; crowd: every GT within that distance of
    one point."""
    g = torch.Generator().manual_seed(seed)
    q = torch.rand(nq, 8, generator=g)
    gt = torch.rand(ngt, 8, generator=g)
    if crowd is not None:
        gt = gt[:1] + crowd * torch.rand(ngt, 8, generator=g)
    c = (q[:, None, :] - gt[None, :, :]).abs().sum(-1)
    if noise:
        c = c + noise * torch.randn(nq, ngt, generator=g)
    return c.float().contiguous()


def _pack(mats, dev, gaps=(3, 0, 17, 1, 5)):
    """The matrices in one buffer at different offsets (filler words between them) + descriptors."""
    parts, desc, off = [], [], 0
    for i, m in enumerate(mats):
        gap = gaps[i % len(gaps)]
        parts.append(torch.full((gap,), 1e30))
        off += gap
        desc.append((off, m.shape[0], m.shape[1], m.shape[1]))
        parts.append(m.reshape(-1))
        off += m.numel()
    return torch.cat(parts).to(dev), torch.tensor(desc, dtype=torch.int64).to(dev)


def _scipy_match_q(m):
    """scipy's assignment in cmt_lsap's match_q form: the query of GT j, or -1."""
    r, c = linear_sum_assignment(m.numpy())
    out = np.full(m.shape[1], -1, dtype=np.int64)
    out[c] = r
    return out


def _solve(mats, dev):
    from projects.mmdet3d_plugin import native_train as T
    costs, desc = _pack(mats, dev)
    mq, mg, st = T.lsap(costs, desc, max_nq=max(m.shape[0] for m in mats), max_ngt=max(m.shape[1] for m in mats))
    torch.cuda.synchronize()
    return mq.cpu().numpy(), mg.cpu().numpy(), st.cpu().numpy()


def _check_inverse(mq_row, mg_row, nq, ngt):
    """match_g is the inverse of match_q, both one-to-one, the smaller side fully assigned."""
    mq_row, mg_row = mq_row[:ngt], mg_row[:nq]
    js = np.nonzero(mq_row >= 0)[0]
    assert len(js) == min(nq, ngt)
    assert len(set(mq_row[js].tolist())) == len(js)
    assert mq_row[js].max(initial=-1) < nq
    want_g = np.full(nq, -1, dtype=np.int64)
    want_g[mq_row[js]] = js
    assert np.array_equal(mg_row, want_g)


def _total(m, mq_row):
    js = np.nonzero(mq_row[:m.shape[1]] >= 0)[0]
    return float(m.double().numpy()[mq_row[js], js].sum())


def test_tie_free_parity_one_launch(dev):
    mats = [_l1_cost(nq, ngt, seed=100 + i) for i, (nq, ngt) in enumerate(PARITY_SHAPES)]
    mq, mg, st = _solve(mats, dev)
    assert st.tolist() == [0] * len(mats)
    for p, m in enumerate(mats):
        nq, ngt = m.shape
        assert np.array_equal(mq[p, :ngt], _scipy_match_q(m)), (p, m.shape)
        _check_inverse(mq[p], mg[p], nq, ngt)
    # match_g is optional: without it match_q is the same
    from projects.mmdet3d_plugin import native_train as T
    costs, desc = _pack(mats, dev)
    mq2, mg2, st2 = T.lsap(costs, desc, max_nq=900, max_ngt=200, want_match_g=False)
    assert mg2 is None and st2.tolist() == [0] * len(mats)
    for p, m in enumerate(mats):
        assert np.array_equal(mq2[p, :m.shape[1]].cpu().numpy(), mq[p, :m.shape[1]])


@pytest.mark.parametrize("shape", [(40, 7), (7, 40), (100, 9), (9, 128), (200, 30), (400, 11), (11, 512), (1100, 20),
                                   (20, 1025), (2048, 64), (2048, 512), (512, 2048)])
def test_every_columns_per_lane_variant_and_the_size_limits(dev, shape):
    """One problem per launch, so max(Nq, ngt) picks each of the solver's column-per-lane
    variants (64, 128, 256, 512, 1024, 2048 columns) in both orientations, up to the limits."""
    m = _l1_cost(*shape, seed=7 + shape[0] + 3 * shape[1])
    mq, mg, st = _solve([m], dev)
    assert st.tolist() == [0]
    assert np.array_equal(mq[0, :shape[1]], _scipy_match_q(m))
    _check_inverse(mq[0], mg[0], *shape)


def test_crowded_gts_long_augmenting_paths(dev):
    """900 x 100 with every GT within 1e-3 of one point: the searches revisit most rows."""
    m = _l1_cost(900, 100, seed=11, noise=0.0, crowd=1e-3)
    mq, mg, st = _solve([m], dev)
    assert st.tolist() == [0]
    _check_inverse(mq[0], mg[0], 900, 100)
    want = _scipy_match_q(m)
    if not np.array_equal(mq[0, :100], want):      # only acceptable when scipy's optimum is not unique
        assert _total(m, mq[0]) == _total(m, want)


def test_integer_ties_equal_total_cost(dev):
    g = torch.Generator().manual_seed(5)
    m = torch.randint(0, 4, (40, 12), generator=g).float()
    mt = m.t().contiguous()
    mq, mg, st = _solve([m, mt], dev)
    assert st.tolist() == [0, 0]
    for p, x in enumerate((m, mt)):
        _check_inverse(mq[p], mg[p], *x.shape)
        assert _total(x, mq[p]) == _total(x, _scipy_match_q(x))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_bad_entries_flag_only_their_problem_and_guards_stay(dev, bad):
    from projects.mmdet3d_plugin import native
    mats = [_l1_cost(70, 5, seed=21), _l1_cost(64, 9, seed=22), _l1_cost(5, 70, seed=23)]
    mats[1][37, 4] = bad
    costs, desc = _pack(mats, dev)
    P, max_nq, max_ngt = 3, 70, 70
    L = native.lib()
    # outputs inside guard words: [guard | match_q P x ld | guard | match_g P x ld | guard | status P | guard]
    G = 64
    buf = torch.full((G + P * max_ngt + G + P * max_nq + G + P + G,), GUARD, dtype=torch.int32, device=dev)
    o_q, o_g, o_s = G, G + P * max_ngt + G, G + P * max_ngt + G + P * max_nq + G
    ws = torch.empty(L.cmt_lsap_workspace_bytes(P, max_nq, max_ngt) // 4, dtype=torch.float32, device=dev)
    a = native.LsapArgs()
    a.P, a.max_nq, a.max_ngt = P, max_nq, max_ngt
    a.cost, a.cost_elems, a.desc = costs.data_ptr(), costs.numel(), desc.data_ptr()
    a.match_q, a.ld_q = buf[o_q:].data_ptr(), max_ngt
    a.match_g, a.ld_g = buf[o_g:].data_ptr(), max_nq
    a.status, a.workspace, a.workspace_bytes = buf[o_s:].data_ptr(), ws.data_ptr(), ws.numel() * 4
    assert L.cmt_lsap(ctypes.byref(a), native._stream()) == 0
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    mq = h[o_q:o_q + P * max_ngt].reshape(P, max_ngt)
    mg = h[o_g:o_g + P * max_nq].reshape(P, max_nq)
    assert h[o_s:o_s + P].tolist() == [0, 1, 0]
    for lo, hi in ((0, G), (o_q + P * max_ngt, o_g), (o_g + P * max_nq, o_s), (o_s + P, len(h))):
        assert (h[lo:hi] == GUARD).all(), (lo, hi)
    for p, m in enumerate(mats):
        nq, ngt = m.shape
        assert (mq[p, ngt:] == GUARD).all() and (mg[p, nq:] == GUARD).all()   # only a problem's own entries
        if p == 1:
            assert (mq[p, :ngt] == -1).all() and (mg[p, :nq] == -1).all()
        else:
            assert np.array_equal(mq[p, :ngt], _scipy_match_q(m))
            _check_inverse(mq[p], mg[p], nq, ngt)


def test_descriptor_outside_the_bounds_is_refused_not_followed(dev):
    """A descriptor larger than the declared maxima, or reaching past the cost buffer, gets
    status 2 and -1 matches; its neighbour is solved."""
    from projects.mmdet3d_plugin import native_train as T
    m = _l1_cost(30, 6, seed=31)
    costs = m.reshape(-1).to(dev)
    desc = torch.tensor([[0, 30, 6, 6], [0, 31, 6, 6], [100, 30, 6, 6], [0, 30, 6, 6]], dtype=torch.int64).to(dev)
    mq, mg, st = T.lsap(costs, desc, max_nq=30, max_ngt=6)
    torch.cuda.synchronize()
    assert st.tolist() == [0, 2, 2, 0]
    want = _scipy_match_q(m)
    for p in (0, 3):
        assert np.array_equal(mq[p].cpu().numpy(), want)
    for p in (1, 2):
        assert (mq[p] == -1).all() and (mg[p] == -1).all()


def test_repeatable_and_follows_new_contents_under_graph_replay(dev):
    from projects.mmdet3d_plugin import native_train as T
    shapes = [(70, 5), (900, 37), (5, 70)]
    mats_a = [_l1_cost(*s, seed=40 + i) for i, s in enumerate(shapes)]
    mats_b = [_l1_cost(*s, seed=50 + i) for i, s in enumerate(shapes)]
    costs_a, desc = _pack(mats_a, dev)
    costs_b, _ = _pack(mats_b, dev)
    costs = costs_a.clone()
    kw = dict(max_nq=900, max_ngt=70)

    def written(out):                              # the entries a launch writes, as one tensor
        mq, mg, st = out
        return torch.cat([st] + [mq[p, :ngt] for p, (_, ngt) in enumerate(shapes)]
                         + [mg[p, :nq] for p, (nq, _) in enumerate(shapes)])
    first = written(T.lsap(costs, desc, **kw))
    second = written(T.lsap(costs, desc, **kw))
    assert torch.equal(first, second)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        T.lsap(costs, desc, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mq, mg, st = T.lsap(costs, desc, **kw)
    for mats, src in ((mats_a, costs_a), (mats_b, costs_b), (mats_a, costs_a)):
        costs.copy_(src)                           # overwritten in place: the replay reads the same address
        graph.replay()
        torch.cuda.synchronize()
        assert st.tolist() == [0, 0, 0]
        for p, m in enumerate(mats):
            assert np.array_equal(mq[p, :m.shape[1]].cpu().numpy(), _scipy_match_q(m)), p
            _check_inverse(mq[p].cpu().numpy(), mg[p].cpu().numpy(), *m.shape)


# ---------------------------------------------------------------------------- head path
def _coop_step(dev):
    """The coop synthetic head of test_training_forward_and_loss_issue_without_host_sync (Nq 64,
    2 layers, 8 GT) and a function running its forward + loss."""
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.models.dense_heads.cmt_head_coop import (get_infrastructure_image_metas,
                                                                          get_vehicle_image_metas)
    head, _, _ = S.build_synthetic_head("cmtcoop_fusion_tumtraf", seed=0, num_query=64, num_layers=2,
                                        grid_size=[256, 256, 40], device=dev)
    head.train()
    head.train_dropout = False
    mv = S.synthetic_metas(1, yaws=S.VEHICLE_YAWS, prefix="vehicle_", pad_shape=(256, 640, 3), seed=7)
    mi = S.synthetic_metas(1, yaws=S.INFRA_YAWS, prefix="infrastructure_", pad_shape=(256, 640, 3), seed=8)
    metas = [dict(mv[0], **mi[0])]
    agents = [(S.synthetic_bev(1, 32, 32, seed=1, device=dev), S.synthetic_img(1, 16, 40, seed=2, device=dev),
               get_vehicle_image_metas(metas)),
              (S.synthetic_bev(1, 32, 32, seed=3, device=dev), S.synthetic_img(3, 16, 40, seed=4, device=dev),
               get_infrastructure_image_metas(metas))]
    gtb, gtl = S.synthetic_gt(1, list(head.pc_range), head.num_classes[0], n=8, seed=5, device=dev)
    rp = torch.rand(64, 3, generator=torch.Generator().manual_seed(6)).to(dev) * 2 - 1
    rp = rp[:min(head.scalar, 64 // 8) * 8]

    def step(poison=False):
        preds = head.forward_train(agents, metas, gtb, gtl, rand_prob=rp)
        if poison:                                  # query 3 of the last layer: NaN logits (every class, as the
            for p in preds:                         # cost reads only the GT labels' columns)
                bad = torch.zeros_like(p["cls_logits"])
                bad[-1, 0, 3, :] = float("nan")
                p["cls_logits"] = p["cls_logits"] + bad
        return head.loss(gtb, gtl, [[p] for p in preds])
    return head, step


def _scipy_must_not_run(*a, **k):
    raise AssertionError("scipy's linear_sum_assignment was called")


def test_head_loss_on_the_device_assignment_equals_the_default_path(dev, monkeypatch):
    from projects.mmdet3d_plugin.models.dense_heads import train_engine as TE
    from projects.mmdet3d_plugin.runtime import options
    head, step = _coop_step(dev)
    want = step()                                   # the default path, scipy on the host
    with options(device_assign=True):
        step()                                      # first use: allocations outside the checked run
    torch.cuda.synchronize()
    monkeypatch.setattr(TE, "linear_sum_assignment", _scipy_must_not_run)
    with options(device_assign=True):
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = step()                            # no event wait, no scipy, no implicit sync
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(head.assign_status.item()) == 0
    assert set(got) == set(want)
    for k in got:
        assert torch.equal(got[k], want[k]), k
    with pytest.raises(AssertionError, match="linear_sum_assignment was called"):
        step()                                      # option off: the patched scipy is what runs


def test_trainer_step_raises_scipys_error_for_a_nan_cost(dev, monkeypatch):
    from projects.mmdet3d_plugin.models.dense_heads import train_engine as TE
    from projects.mmdet3d_plugin.runtime import options
    from projects.mmdet3d_plugin.trainer import Trainer
    head, step = _coop_step(dev)
    monkeypatch.setattr(TE, "linear_sum_assignment", _scipy_must_not_run)
    with Trainer(head) as trainer, options(device_assign=True):
        trainer.step(step())                        # a clean step passes the status check
        assert trainer.step_count == 1
        weights = trainer.fp.flat.clone()
        with pytest.raises(ValueError, match="cost matrix contains invalid numeric entries"):
            trainer.step(step(poison=True))
        assert trainer.step_count == 1 and torch.equal(trainer.fp.flat, weights)   # the optimiser did not run
