"""Native box decode (cmt_box_decode via MultiTaskBBoxCoder / get_bboxes)
vs the oracle's restatement of MultiTaskBBoxCoder.decode + get_bboxes
(oracle/cmt_oracle.py decode)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("center", "height", "dim", "rot", "vel")
WIDTH = {"center": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2}


def _preds(B, Nq, class_split, seed, ties=False):
    g = torch.Generator().manual_seed(seed)
    preds = []
    for n in class_split:
        d = {k: torch.randn(6, B, Nq, w, generator=g) * (30 if k == "center" else 1) for k, w in WIDTH.items()}
        d["cls_logits"] = torch.randn(6, B, Nq, n, generator=g) * 2
        if ties:   # a block of equal logits straddling the k-th value
            d["cls_logits"][-1, :, :40, 0] = 0.25
        preds.append(d)
    return preds


@pytest.mark.parametrize("B,Nq,split,max_num,thr,ties", [(1, 900, [10], 300, None, False),
                                                        (2, 300, [3, 4], 100, 0.3, False),
                                                        (1, 200, [10], 150, None, True),
                                                        (3, 400, [7], 350, 0.05, False)])
def test_native_decode_matches_oracle(dev, B, Nq, split, max_num, thr, ties):
    from oracle import cmt_oracle as O
    from projects.mmdet3d_plugin.core.bbox.coders import MultiTaskBBoxCoder
    preds = _preds(B, Nq, split, seed=B * 100 + Nq, ties=ties)
    ncls = sum(split)
    pcr = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
    ref = O.decode(preds, ncls, max_num=max_num, post_center_range=pcr, score_threshold=thr)
    coder = MultiTaskBBoxCoder(pc_range=[-54, -54, -5, 54, 54, 3], post_center_range=pcr, max_num=max_num,
                               score_threshold=thr, num_classes=ncls)
    got = coder.decode([[{k: v.to(dev) for k, v in d.items()}] for d in preds])
    for b in range(B):
        r, g = ref[b], got[b]
        gb = g["bboxes"].cpu().clone()
        gb[:, 2] = gb[:, 2] - gb[:, 5] * 0.5          # the z-shift get_bboxes applies (oracle.decode includes it)
        assert g["scores"].shape == r["scores"].shape
        assert torch.allclose(g["scores"].cpu(), r["scores"], atol=1e-6)
        assert torch.equal(g["labels"].cpu(), r["labels"].long())
        assert torch.allclose(gb, r["bboxes"], atol=1e-4, rtol=1e-5)
        if len(g["scores"]) > 1:
            assert (g["scores"][:-1] >= g["scores"][1:]).all()


# ---------------------------------------------------------------------------
# cmt_box_decode called directly (native.box_decode) against a torch restatement of the
# kernel's contract: code 8, the limits in both dimensions, strided batches, the tie rule.
# ---------------------------------------------------------------------------
PCR = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]


def _lattice_logits(B, n, g, lo=-6.0, hi=6.0):
    """distinct float32 logits per sample: a random permutation of n points of step (hi - lo) / n,
    offset by half a step (no 0.0 for a symmetric range)"""
    step = (hi - lo) / n
    return torch.stack([(torch.randperm(n, generator=g).double() + 0.5) * step + lo for _ in range(B)]).float()


def _threshold_gap(logits, at):
    """open a gap of 0.1 in the logits above `at` and put the score threshold in its middle, so
    that no score lies within 1e-5 of it however dense the lattice is"""
    return torch.where(logits > at, logits + 0.1, logits), torch.sigmoid(torch.tensor(at + 0.05)).item()


def _boxes(B, rows, code, g, outside=False):
    bb = torch.randn(B, rows, code, generator=g)
    c = (torch.rand(B, rows, 3, generator=g) * 2 - 1) * torch.tensor([70.0, 70.0, 12.0])
    if outside:
        c[..., 0] = 61.2 + 0.5 + torch.rand(B, rows, generator=g)
    lim = torch.tensor(PCR[3:])
    near = (c.abs() - lim).abs() < 2e-3          # keep every centre clear of the range bounds
    c = torch.where(near, c + 0.01 * torch.sign(c), c)
    bb[..., :3] = c
    return bb


def _decode_ref(logits, bbox, class_task, Nq, ncls, max_num, thr):
    """per sample (boxes [n, code-1] f64, scores [n] f64, labels [n]); asserts the input conditions"""
    res = []
    ct = torch.tensor(class_task)
    pcr = torch.tensor(PCR, dtype=torch.float64)
    for b in range(logits.shape[0]):
        lg = logits[b]
        assert not (lg == 0).any()
        idx = torch.sort(-lg, stable=True).indices[:max_num]          # (-logit, flat index)
        score = torch.sigmoid(lg[idx].double())
        label = idx % ncls
        q = torch.div(idx, ncls, rounding_mode="floor")
        bp = bbox[b][ct[label] * Nq + q].double()
        box = torch.cat([bp[:, :3], bp[:, 3:6].exp(), torch.atan2(bp[:, 6:7], bp[:, 7:8]), bp[:, 8:]], 1)
        assert torch.minimum((box[:, :3] - pcr[:3]).abs(), (box[:, :3] - pcr[3:]).abs()).min() > 1e-3
        keep = ((box[:, :3] >= pcr[:3]) & (box[:, :3] <= pcr[3:])).all(1)
        if thr is not None:
            assert (score - thr).abs().min() > 1e-5
            keep &= score > thr
        res.append((box[keep], score[keep], label[keep]))
    return res


def _decode_check(dev, logits, bbox, class_task, Nq, ncls, max_num, thr=None, distinct=True):
    from projects.mmdet3d_plugin import native
    if distinct:
        for b in range(logits.shape[0]):
            assert torch.unique(logits[b]).numel() == logits.shape[1]
    ref = _decode_ref(logits.cpu(), bbox.cpu(), class_task, Nq, ncls, max_num, thr)
    boxes, scores, labels, count = native.box_decode(
        logits.to(dev) if not logits.is_cuda else logits, bbox.to(dev) if not bbox.is_cuda else bbox,
        torch.tensor(class_task, dtype=torch.int32, device=dev), Nq=Nq, ncls=ncls, max_num=max_num,
        post_center_range=PCR, score_threshold=thr)
    assert boxes.shape == (logits.shape[0], max_num, bbox.shape[-1] - 1)
    counts = count.cpu().tolist()
    for b, (rb, rs, rl) in enumerate(ref):
        n = counts[b]
        assert n == len(rs)
        assert torch.allclose(scores[b, :n].cpu().double(), rs, atol=1e-6, rtol=0)
        assert torch.equal(labels[b, :n].cpu().long(), rl)
        assert torch.allclose(boxes[b, :n].cpu().double(), rb, atol=1e-4, rtol=1e-5)
    return counts


@pytest.mark.parametrize("code,B,Nq,ncls,max_num,thr_at", [(8, 2, 50, 4, 60, None),      # 7 output columns, no velocity
                                                       (8, 2, 50, 4, 60, 3.0),       # a threshold inside the top-k
                                                       (10, 2, 50, 4, 200, None),    # max_num == Nq * ncls
                                                       (10, 2, 50, 4, 1, None),
                                                       (10, 1, 4096, 8, 1024, 5.8)])   # both documented maxima
def test_box_decode_direct(dev, code, B, Nq, ncls, max_num, thr_at):
    g = torch.Generator().manual_seed(code * 1000 + Nq + max_num)
    logits, thr = _lattice_logits(B, Nq * ncls, g), None
    if thr_at is not None:
        logits, thr = _threshold_gap(logits, thr_at)
    bbox = _boxes(B, Nq, code, g)
    counts = _decode_check(dev, logits, bbox, [0] * ncls, Nq, ncls, max_num, thr)
    assert max(counts) > 0


def test_box_decode_two_tasks_strided(dev):
    """class_task maps labels onto two bbox blocks; logits and bbox are batch slices of larger,
    NaN-filled buffers (stride(0) beyond the row)."""
    g = torch.Generator().manual_seed(21)
    B, Nq, ncls, max_num, task = 3, 40, 5, 70, [0, 0, 1, 1, 1]
    lbig = torch.full((B, Nq * ncls + 13), float("nan"), device=dev)
    bbig = torch.full((B, 2 * Nq + 3, 10), float("nan"), device=dev)
    lg, thr = _threshold_gap(_lattice_logits(B, Nq * ncls, g), 2.2)
    lbig[:, :Nq * ncls] = lg.to(dev)
    bbig[:, :2 * Nq] = _boxes(B, 2 * Nq, 10, g).to(dev)
    logits, bbox = lbig[:, :Nq * ncls], bbig[:, :2 * Nq]
    assert logits.stride(0) > Nq * ncls and bbox.stride(0) > 2 * Nq * 10
    counts = _decode_check(dev, logits, bbox, task, Nq, ncls, max_num, thr)
    assert max(counts) > 0


def test_box_decode_all_negative_logits(dev):
    """every key takes the sign-bit branch of the order-preserving map"""
    g = torch.Generator().manual_seed(22)
    B, Nq, ncls, max_num = 2, 50, 4, 60
    logits = _lattice_logits(B, Nq * ncls, g, lo=-9.0, hi=-1.0)
    assert (logits < 0).all()
    counts = _decode_check(dev, logits, _boxes(B, Nq, 10, g), [0] * ncls, Nq, ncls, max_num)
    assert max(counts) > 0


def test_box_decode_all_rejected(dev):
    g = torch.Generator().manual_seed(23)
    B, Nq, ncls, max_num = 2, 50, 4, 60
    counts = _decode_check(dev, _lattice_logits(B, Nq * ncls, g), _boxes(B, Nq, 10, g, outside=True), [0] * ncls,
                           Nq, ncls, max_num)
    assert counts == [0, 0]


def test_box_decode_ties_lowest_index(dev):
    """64 equal logits on ranks 30..93 straddle max_num = 60: the 30 of lowest flat index enter"""
    g = torch.Generator().manual_seed(24)
    B, Nq, ncls, max_num = 2, 50, 4, 60
    logits = _lattice_logits(B, Nq * ncls, g)
    for b in range(B):
        order = torch.sort(-logits[b]).indices
        logits[b, order[30:94]] = logits[b, order[30]].item()
        assert (logits[b] == logits[b, order[30]]).sum() == 64
    # centres well inside, so that every rank is emitted and the tie rule shows in the labels
    bbox = _boxes(B, Nq, 10, g)
    bbox[..., :3] = bbox[..., :3] * 0.1
    counts = _decode_check(dev, logits, bbox, [0] * ncls, Nq, ncls, max_num, distinct=False)
    assert counts == [max_num] * B


@pytest.mark.parametrize("Nq,ncls,code,max_num", [(1000, 2, 10, 1025), (32769, 1, 10, 16), (10, 2, 10, 21),
                                                  (50, 4, 9, 60)])
def test_box_decode_rejects_limits(dev, Nq, ncls, code, max_num):
    from projects.mmdet3d_plugin import native
    logits = torch.zeros(1, Nq * ncls, device=dev)
    bbox = torch.zeros(1, Nq, code, device=dev)
    with pytest.raises(RuntimeError):
        native.box_decode(logits, bbox, torch.zeros(ncls, dtype=torch.int32, device=dev), Nq=Nq, ncls=ncls,
                          max_num=max_num, post_center_range=PCR)
