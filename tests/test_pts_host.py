"""Host side of cmt_pts_prepare: the contract of tests/_pts_ref.py against the reference's own expressions run
literally on the CPU, the sweep choice and config helpers of native_pts, the ABI mirror and the argument errors.
No GPU needed.

Bounds of the comparison with the reference's expressions (4 096 seeded rows over +-80 m):

* sweep rotation: the reference's ``pts[:, :3] @ R.T`` is a float64 matmul whose order and fusing the BLAS
  chooses.  Two float64 evaluations of a 3-term dot product differ by a few float64 ulps, far below half a float32
  ulp, so after the one rounding to float32 they are equal or neighbours: 1 float32 ulp.
* sweep translation ``+= t``: the float64 sums differ by what q differed, and each is rounded once more, so
  |dp| <= ulp32(q) + ulp32(p).
* agent transform ``tensor @ rot32; += t32`` in float32: four roundings per coordinate in either order, so
  |dp| <= 2^-22 (|r0 x| + |r1 y| + |r2 z| + |t|).
* keep masks: rows are drawn by rejection so that no contract coordinate lies within the agent bound (plus the
  sweep bound carried through the rotation) of a range face; then the masks must be equal.  remove_close acts on
  the raw row, where both sides compare the same float32 numbers.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _pts_ref as R

REF_CONFIGS = "/root/reference/projects/configs"
RANGE = [-72.0, -72.0, -8.0, 72.0, 72.0, 0.0]
N_ROWS = 4096


_rigid = R.rigid


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _literal_sweep(pts, rot, trans):
    """loading_coop.py:261-264, literally"""
    p = np.copy(pts)
    p[:, :3] = p[:, :3] @ rot.T
    q = np.copy(p[:, :3])
    p[:, :3] += trans
    return q, p[:, :3]


def _literal_agent(xyz, v2i):
    """VehiclePointsToInfraCoords: BasePoints.rotate(v2i_rot.T) then translate(v2i_trans) on a float32 tensor"""
    t = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).clone()
    rot_mat_T = t.new_tensor(v2i[:3, :3].T)
    t[:, :3] = t[:, :3] @ rot_mat_T
    t[:, :3] += t.new_tensor(v2i[:3, 3])
    return t.numpy()


def _literal_range(xyz, rng):
    """in_range_3d of BasePoints, strict"""
    r = np.array(rng, dtype=np.float32)
    t = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32))
    m = ((t[:, 0] > r[0]) & (t[:, 1] > r[1]) & (t[:, 2] > r[2]) & (t[:, 0] < r[3]) & (t[:, 1] < r[4]) & (t[:, 2] < r[5]))
    return m.numpy()


def _agent_bound(xyz, v2i):
    r = np.abs(v2i[:3, :3].astype(np.float32).astype(np.float64))
    a = np.abs(xyz.astype(np.float64))
    return 2.0 ** -22 * (a @ r.T + np.abs(v2i[:3, 3].astype(np.float32).astype(np.float64)))


def test_sweep_transform_against_numpy_matmul():
    rng = np.random.default_rng(11)
    pts = rng.uniform(-80, 80, (N_ROWS, 5)).astype(np.float32)
    rot, trans = _rigid(rng, 3.0)
    q_ref, p_ref = _literal_sweep(pts, rot, trans)
    q_con = R.sweep_xform(pts[:, :3], rot, np.zeros(3))
    p_con = R.sweep_xform(pts[:, :3], rot, trans)
    dq = np.abs(q_ref.astype(np.float64) - q_con.astype(np.float64))
    dp = np.abs(p_ref.astype(np.float64) - p_con.astype(np.float64))
    print(f"sweep: q differs in {int((dq > 0).sum())} of {dq.size} coordinates, max {dq.max():.3e}; p max {dp.max():.3e}")
    assert np.all(dq <= np.maximum(_ulp32(q_ref), _ulp32(q_con)))
    assert np.all(dp <= np.maximum(_ulp32(q_ref), _ulp32(q_con)) + np.maximum(_ulp32(p_ref), _ulp32(p_con)))


def test_agent_transform_against_torch_matmul():
    rng = np.random.default_rng(12)
    xyz = rng.uniform(-80, 80, (N_ROWS, 3)).astype(np.float32)
    rot, trans = _rigid(rng, 30.0)
    v2i = np.eye(4)
    v2i[:3, :3], v2i[:3, 3] = rot, trans
    ref = _literal_agent(xyz, v2i)
    con = R.agent_xform(xyz, v2i[:3, :3].astype(np.float32), v2i[:3, 3].astype(np.float32))
    d = np.abs(ref.astype(np.float64) - con.astype(np.float64))
    bound = _agent_bound(xyz, v2i)
    print(f"agent: {int((d > 0).sum())} of {d.size} coordinates differ, max {d.max():.3e}, smallest slack "
          f"{(bound - d).min():.3e}")
    assert np.all(d <= bound)


def test_whole_chain_keep_masks_and_rows():
    """key frame + 2 sweeps (one with remove_close), agent transform, range filter: the reference's chain literally
    against the contract, on rows drawn so that no coordinate is within the bound of a range face"""
    rng = np.random.default_rng(13)
    v2i = np.eye(4)
    v2i[:3, :3], v2i[:3, 3] = _rigid(rng, 20.0)
    v2i[2, 3] = rng.uniform(-1.0, 1.0)   # the z range is 8 m high
    sweeps = [_rigid(rng, 2.0) for _ in range(2)]
    key_ts, sweep_ts = 1_700_000_000_400_000, [1_700_000_000_300_000, 1_700_000_000_150_000]
    use_dim = [0, 1, 2, 3, 4]
    per = [N_ROWS - 2 * (N_ROWS // 3), N_ROWS // 3, N_ROWS // 3]

    def build(raw):
        """raw: list of 3 float32 [n, 5] arrays -> (contract rows incl. dropped, contract mask, literal rows, literal mask)"""
        segs = [R.seg(raw[0], time_col=4, time=0.0)]
        lit = [np.copy(raw[0])]
        lit[0][:, 4] = 0
        lit_keep = [np.ones(len(raw[0]), bool)]
        for i, (rot, trans) in enumerate(sweeps):
            lag = key_ts / 1e6 - sweep_ts[i] / 1e6
            close = 1.0 if i == 0 else 0.0
            segs.append(R.seg(raw[i + 1], rot, trans, close, 4, np.float32(lag)))
            p = np.copy(raw[i + 1])
            nc = np.ones(len(p), bool)
            if close:
                nc = np.logical_not(np.logical_and(np.abs(p[:, 0]) < 1.0, np.abs(p[:, 1]) < 1.0))
            p[:, :3] = p[:, :3] @ rot.T
            p[:, :3] += trans
            p[:, 4] = lag
            lit.append(p)
            lit_keep.append(nc)
        lit_rows = np.concatenate(lit, 0)[:, use_dim]
        lit_rows[:, :3] = _literal_agent(lit_rows[:, :3], v2i)
        lit_mask = np.concatenate(lit_keep) & _literal_range(lit_rows[:, :3], RANGE)
        # the contract, all rows (no filter) and its mask
        nofilter = [dict(s, remove_close=0.0) for s in segs]
        all_rows, _ = R.reference(nofilter, use_dim, (v2i[:3, :3], v2i[:3, 3]), None)
        _, con_mask = R.reference(segs, use_dim, (v2i[:3, :3], v2i[:3, 3]), RANGE)
        return all_rows, con_mask, lit_rows, lit_mask

    def unsafe(all_rows):
        """rows with a coordinate within 1e-4 m of a range face.  That covers the bound asserted below: the agent
        step's 2^-22 (|r0 x| + |r1 y| + |r2 z| + |t|) <= 2^-22 * 200 = 4.8e-5 m at these coordinates, plus the sweep
        step's 2 float32 ulps at < 128 m (2^-16 m) carried through a rotation, 2.6e-5 m"""
        faces = np.array(RANGE, np.float64)
        d = np.minimum(np.abs(all_rows[:, :3].astype(np.float64) - faces[:3]), np.abs(all_rows[:, :3] - faces[3:]))
        return np.any(d < 1e-4, axis=1)

    raw = [rng.uniform(-80, 80, (n, 5)).astype(np.float32) for n in per]
    for k in range(3):
        raw[k][:, 2] = rng.uniform(-10, 2, per[k]).astype(np.float32)
        raw[k][:16, :2] = rng.uniform(-1.5, 1.5, (16, 2)).astype(np.float32)   # some rows near the sensor
    for _ in range(20):
        all_rows, con_mask, lit_rows, lit_mask = build(raw)
        bad = unsafe(all_rows)
        if not bad.any():
            break
        off = 0
        for k in range(3):
            b = bad[off:off + per[k]]
            raw[k][b, :2] = rng.uniform(-80, 80, (int(b.sum()), 2)).astype(np.float32)
            raw[k][b, 2] = rng.uniform(-10, 2, int(b.sum())).astype(np.float32)
            off += per[k]
    excluded = float(unsafe(all_rows).mean())
    assert excluded == 0.0, f"{excluded:.4%} of the rows are still within the bound of a range face"
    assert all_rows.shape[0] == N_ROWS
    assert np.array_equal(con_mask, lit_mask)
    assert 0.2 < con_mask.mean() < 0.95, "the case must both keep and drop"
    d = np.abs(all_rows[:, :3].astype(np.float64) - lit_rows[:, :3].astype(np.float64))
    # the sweep step's error (ulp(q) + ulp(p) <= 2 ulp at < 128 m = 2^-16 m) passes through a rotation (factor
    # <= sqrt(3) in any coordinate) and the agent step adds its own four roundings
    bound = _agent_bound(lit_rows[:, :3], v2i) + np.sqrt(3.0) * 2 * 2.0 ** -17
    print(f"chain: max coordinate distance {d.max():.3e} m, smallest slack {(bound - d).min():.3e}; kept "
          f"{int(con_mask.sum())} of {N_ROWS}")
    assert np.all(d <= bound)
    assert np.array_equal(all_rows[:, 3:], lit_rows[:, 3:].astype(np.float32))   # intensity and time lag: copies
    assert all_rows[per[0], 4] == np.float32(key_ts / 1e6 - sweep_ts[0] / 1e6)


def test_reference_module_known_answers():
    p = np.array([[0.5, 0.5, 0, 7, 9], [2, 0.5, 0, 7, 9], [np.nan, 0.1, 0, 7, 9], [1.0, 1.0, 0, 7, 9]], np.float32)
    kept, mask = R.reference([R.seg(p, remove_close=1.0)], [0, 1, 2, 4])
    assert mask.tolist() == [False, True, True, True] and kept.shape == (3, 4) and np.all(kept[:, 3] == 9)
    kept, mask = R.reference([R.seg(p, time_col=3, time=0.25)], [0, 1, 2, 3], rng=[0, 0, -1, 2, 2, 1])
    assert mask.tolist() == [True, False, False, True] and np.all(kept[:, 3] == 0.25)   # x = 2 lies on the face
    out, count = R.padded([R.seg(p, remove_close=1.0)], [0, 1, 2])
    assert count == 3 and np.all(out[3] == 0x7FC00000) and out.shape == (4, 3)
    rot = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    got = R.sweep_xform(np.array([[1, 2, 3]], np.float32), rot, [10, 20, 30])
    assert got.tolist() == [[8.0, 21.0, 33.0]]
    got = R.agent_xform(np.array([[1, 2, 3]], np.float32), rot, [10, 20, 30])
    assert got.tolist() == [[8.0, 21.0, 33.0]]


# ---- native_pts' host helpers ------------------------------------------------------------------------------------
def _sweeps(n):
    return [dict(points=f"s{i}", sensor2lidar_rotation=np.eye(3) * (i + 1), sensor2lidar_translation=np.full(3, i),
                 timestamp=1_000_000_000 - 50_000 * (i + 1)) for i in range(n)]


def test_sweep_segments():
    from projects.mmdet3d_plugin import native_pts as NP
    ts = 1_000_000_000
    key = dict(points="key", time_col=4, time=0.0)
    # fewer sweeps than sweeps_num: all, in order
    segs = NP.sweep_segments("key", _sweeps(3), ts, sweeps_num=10)
    assert segs[0] == key and [s["points"] for s in segs[1:]] == ["s0", "s1", "s2"]
    for i, s in enumerate(segs[1:]):
        assert np.array_equal(s["rotation"], np.eye(3) * (i + 1)) and np.array_equal(s["translation"], np.full(3, i))
        assert s["remove_close"] == 0.0 and s["time_col"] == 4
        assert s["time"] == float(np.float32(ts / 1e6 - (ts - 50_000 * (i + 1)) / 1e6))
    assert abs(segs[1]["time"] - 0.05) < 1e-6
    # more: the first sweeps_num in test mode; the random choice is not built
    segs = NP.sweep_segments("key", _sweeps(5), ts, sweeps_num=2, remove_close=True, time_dim=3)
    assert [s["points"] for s in segs] == ["key", "s0", "s1"] and segs[0] == dict(points="key", time_col=3, time=0.0)
    assert all(s["remove_close"] == 1.0 and s["time_col"] == 3 for s in segs[1:])
    with pytest.raises(NotImplementedError):
        NP.sweep_segments("key", _sweeps(5), ts, sweeps_num=2, test_mode=False)
    # the coop loader writes the lag to column 4 whatever time_dim is
    segs = NP.sweep_segments("key", _sweeps(1), ts, time_dim=3, coop=True)
    assert segs[0]["time_col"] == 3 and segs[1]["time_col"] == 4
    # none
    assert NP.sweep_segments("key", [], ts) == [key]
    segs = NP.sweep_segments("key", [], ts, pad_empty_sweeps=True, sweeps_num=3, remove_close=True)
    assert segs == [key] + [dict(points="key", remove_close=1.0, time_col=4, time=0.0)] * 3
    segs = NP.sweep_segments("key", [], ts, pad_empty_sweeps=True, sweeps_num=2)
    assert segs == [key] + [dict(points="key", remove_close=0.0, time_col=4, time=0.0)] * 2
    for kw in (dict(reduce_beams=16), dict(load_augmented="mvp")):
        with pytest.raises(NotImplementedError):
            NP.sweep_segments("key", [], ts, **kw)


NUS = dict(load_dim=5, use_dim=[0, 1, 2, 3, 4], sweeps_num=10, remove_close=False, time_dim=4, point_cloud_range=None,
           coop=False)
COOP = dict(NUS, point_cloud_range=[-72.0, -72.0, -8.0, 72.0, 72.0, 0.0], coop=True)
PLANS = {
    "CMTCoop_TUMTraf/camera/coop/cmt_camera_vov_1600x640_cbgs_a9coop_pretrained.py": None,
    "CMTCoop_TUMTraf/camera/infra/cmt_camera_vov_1600x640_cbgs_a9coop_infrastructure_pretrained.py": None,
    "CMTCoop_TUMTraf/camera/vehicle/cmt_camera_vov_1600x640_cbgs_a9coop_vehicle_pretrained.py": None,
    "CMTCoop_TUMTraf/fusion/coop/cmt_voxel0075_vov_1600x640_cbgs_a9coop_pretrained.py": COOP,
    "CMTCoop_TUMTraf/fusion/infra/cmt_voxel0075_vov_1600x640_cbgs_a9coop_infrastructure_pretrained.py": COOP,
    "CMTCoop_TUMTraf/fusion/vehicle/cmt_voxel0075_vov_1600x640_cbgs_a9coop_vehicle_pretrained.py": COOP,
    "CMTCoop_TUMTraf/lidar/coop/cmt_lidar_voxel0075_cbgs_a9coop_pretrained.py": COOP,
    "CMTCoop_TUMTraf/lidar/infra/cmt_lidar_voxel0075_cbgs_a9coop_infrastructure_pretrained.py": COOP,
    "CMTCoop_TUMTraf/lidar/vehicle/cmt_lidar_voxel0075_cbgs_a9coop_vehicle_pretrained.py": COOP,
    "CMT_Nuscenes/camera/cmt_camera_vov_1600x640_cbgs.py": None,
    "CMT_Nuscenes/fusion/cmt_voxel0075_vov_1600x640_cbgs.py": NUS,
    "CMT_Nuscenes/fusion/cmt_voxel0100_r50_800x320_cbgs.py": NUS,
    "CMT_Nuscenes/lidar/cmt_lidar_voxel0075_cbgs.py": NUS,
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_points_plan_from_reference_config(name):
    if not os.path.isdir(REF_CONFIGS):
        pytest.skip("reference checkout not present")
    from projects.mmdet3d_plugin import native_pts as NP
    from projects.mmdet3d_plugin.config import load_config
    assert NP.points_plan_from_config(load_config(os.path.join(REF_CONFIGS, name))) == PLANS[name]


@pytest.mark.parametrize("name", ["cmt_lidar_nus", "cmt_fusion_nus", "cmtcoop_fusion_tumtraf", "cmtcoop_lidar_tumtraf"])
def test_points_plan_from_package_config(name):
    from projects.mmdet3d_plugin import native_pts as NP
    from projects.mmdet3d_plugin import synthetic as S
    from projects.mmdet3d_plugin.config import load_config
    plan = NP.points_plan_from_config(load_config(os.path.join(S.CONFIG_DIR, name + ".py")))
    assert plan == (COOP if name.startswith("cmtcoop") else NUS)


def test_points_plan_from_a_plain_dict():
    from projects.mmdet3d_plugin import native_pts as NP
    ident = dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0])
    steps = [dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=6, use_dim=6),
             dict(type="LoadPointsFromMultiSweeps", load_dim=6, sweeps_num=4, use_dim=[0, 1, 2, 5, 3], remove_close=True,
                  time_dim=5),
             dict(type="MultiScaleFlipAug3D", transforms=[ident, dict(type="PointsRangeFilter",
                                                                     point_cloud_range=[-1, -2, -3, 1, 2, 3])])]
    cfg = dict(data=dict(test=dict(pipeline=steps)))
    assert NP.points_plan_from_config(cfg) == dict(load_dim=6, use_dim=[0, 1, 2, 5, 3], sweeps_num=4, remove_close=True,
                                                   time_dim=5, point_cloud_range=[-1.0, -2.0, -3.0, 1.0, 2.0, 3.0],
                                                   coop=False)
    # camera only; a key frame alone; a file loader that drops columns in front of the sweeps; a real augmentation
    assert NP.points_plan_from_config(dict(data=dict(test=dict(pipeline=[dict(type="LoadMultiViewImageFromFiles")])))) is None
    alone = NP.points_plan_from_config(dict(data=dict(test=dict(pipeline=steps[:1]))))
    assert alone["sweeps_num"] == 0 and alone["use_dim"] == [0, 1, 2, 3, 4, 5] and alone["point_cloud_range"] is None
    steps[0]["use_dim"] = [0, 1, 2, 4]
    with pytest.raises(ValueError, match="drops columns"):
        NP.points_plan_from_config(cfg)
    steps[0]["use_dim"] = 6
    ident["rot_range"] = [-0.3925, 0.3925]
    with pytest.raises(ValueError, match="not the identity"):
        NP.points_plan_from_config(cfg)
    del ident["rot_range"]
    with pytest.raises(ValueError, match="not the identity"):
        NP.points_plan_from_config(cfg)


def test_lidar2img_to_infra():
    from projects.mmdet3d_plugin import native_pts as NP
    rng = np.random.default_rng(5)
    v2i = np.eye(4)
    v2i[:3, :3], v2i[:3, 3] = _rigid(rng, 20.0)
    M = rng.normal(size=(3, 4, 4))
    got = NP.lidar2img_to_infra(M, v2i)
    assert got.dtype == np.float64 and got.shape == (3, 4, 4)
    # a vehicle-frame point and its infrastructure-frame image project alike
    p = np.array([3.0, -2.0, 1.0, 1.0])
    assert np.allclose(got @ (v2i @ p), M @ p, rtol=0, atol=1e-9)
    assert np.array_equal(NP.lidar2img_to_infra(M[0], v2i), got[0])
    with pytest.raises(ValueError):
        NP.lidar2img_to_infra(np.eye(3), v2i)


def test_prepare_points_argument_errors():
    from projects.mmdet3d_plugin import native_pts as NP
    p = torch.zeros((4, 5))
    for segs, kw in (([], dict(use_dim=5)),
                     ([dict(points=p)] * 17, dict(use_dim=5)),
                     ([dict(points=p)], dict(use_dim=[0, 2, 1, 3])),
                     ([dict(points=p)], dict(use_dim=[0, 1, 2, 5])),
                     ([dict(points=p)], dict(use_dim=5, load_dim=9)),
                     ([dict(points=p.double())], dict(use_dim=5)),
                     ([dict(points=p[:, :4])], dict(use_dim=4)),
                     ([dict(points=p, time_col=5, time=0.0)], dict(use_dim=5)),
                     ([dict(points=p, time_col=4)], dict(use_dim=5)),
                     ([dict(points=p, remove_close=-1.0)], dict(use_dim=5)),
                     ([dict(points=p, rotation=np.eye(2))], dict(use_dim=5)),
                     ([dict(points=p, rotation=np.full((3, 3), np.nan))], dict(use_dim=5)),
                     ([dict(points=p, colour=1)], dict(use_dim=5)),
                     ([dict(points=p)], dict(use_dim=5, agent_transform=np.eye(3))),
                     ([dict(points=p)], dict(use_dim=5, point_cloud_range=[0, 0, 0, 1, 1, 0])),
                     ([dict(points=p)], dict(use_dim=5, point_cloud_range=[0, 0, 0, 1, np.inf, 1])),
                     ([dict(points=p)], dict(use_dim=5))):   # a CPU tensor: no CPU path
        with pytest.raises(ValueError):
            NP.prepare_points(segs, **kw)


# ---- ABI and errors ----------------------------------------------------------------------------------------------
def _lib():
    from projects.mmdet3d_plugin import native
    if not native.available():
        pytest.skip("libcmt_hip.so not built")
    return native, native.lib()


def test_pts_prepare_abi():
    native, L = _lib()
    assert L.cmt_abi_version() == 25
    for name in ("cmt_pts_prepare", "cmt_pts_prepare_args_size", "cmt_pts_prepare_workspace_bytes",
                 "cmt_pts_prepare_tile_rows"):
        assert hasattr(L, name)
    assert L.cmt_pts_prepare_args_size() == ctypes.sizeof(native.PtsPrepareArgs)
    assert native.STRUCTS["pts_prepare"] is native.PtsPrepareArgs
    T = L.cmt_pts_prepare_tile_rows()
    assert T > 0 and T % 64 == 0
    assert L.cmt_pts_prepare_workspace_bytes(0) == 0
    assert L.cmt_pts_prepare_workspace_bytes(1) == 4 and L.cmt_pts_prepare_workspace_bytes(T) == 4
    assert L.cmt_pts_prepare_workspace_bytes(T + 1) == 8 and L.cmt_pts_prepare_workspace_bytes(300000) == 4 * -(-300000 // T)


def _args(native, null=True, **kw):
    """a valid call on 100 rows in 2 segments; the device pointers are null (``null``) or fake, never dereferenced:
    every case is rejected before any device work"""
    a = native.PtsPrepareArgs()
    a.n_total, a.S, a.load_dim, a.F_out = 100, 2, 5, 4
    for i, v in enumerate([0, 60] + [100] * 15):
        a.seg_start[i] = v
    for j, u in enumerate([0, 1, 2, 4]):
        a.use_dim[j] = u
    for s in range(2):
        a.seg[s].time_col = -1
    a.seg[1].has_sweep_xform = 1
    for k in (0, 4, 8):
        a.seg[1].rot[k] = 1.0
    a.has_range = 1
    for k, v in enumerate([-1, -1, -1, 1, 1, 1]):
        a.range[k] = v
    if not null:
        a.src, a.dst, a.count, a.workspace = 4096, 8192, 12288, 16384
        a.workspace_bytes = 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _seg_field(native, s, **kw):
    a = _args(native)
    for k, v in kw.items():
        setattr(a.seg[s], k, v)
    return a


def _arr(native, name, idx, val, **kw):
    a = _args(native, **kw)
    getattr(a, name)[idx] = val
    return a


REJECTS = {
    "S 0": (lambda n: _args(n, S=0), "S must be"),
    "S 17": (lambda n: _args(n, S=17), "S must be"),
    "load_dim 2": (lambda n: _args(n, load_dim=2), "load_dim"),
    "load_dim 9": (lambda n: _args(n, load_dim=9), "load_dim"),
    "F_out 2": (lambda n: _args(n, F_out=2), "F_out"),
    "F_out 9": (lambda n: _args(n, F_out=9), "F_out"),
    "use_dim beyond load_dim": (lambda n: _arr(n, "use_dim", 3, 5), "use_dim"),
    "use_dim negative": (lambda n: _arr(n, "use_dim", 3, -1), "use_dim"),
    "use_dim not 0 1 2": (lambda n: _arr(n, "use_dim", 1, 2), "start with 0, 1, 2"),
    "seg_start decreasing": (lambda n: _arr(n, "seg_start", 1, 101), "seg_start"),
    "seg_start first": (lambda n: _arr(n, "seg_start", 0, 1), "seg_start"),
    "seg_start end": (lambda n: _args(n, n_total=99), "seg_start"),
    "n_total 2^31": (lambda n: _arr(n, "seg_start", 2, 2 ** 31, n_total=2 ** 31), "n_total"),
    "n_total negative": (lambda n: _args(n, n_total=-1), "n_total"),
    "time_col": (lambda n: _seg_field(n, 1, time_col=5), "time_col"),
    "time_col -2": (lambda n: _seg_field(n, 0, time_col=-2), "time_col"),
    "close_radius negative": (lambda n: _seg_field(n, 0, close_radius=-0.5), "close_radius"),
    "close_radius nan": (lambda n: _seg_field(n, 1, close_radius=float("nan")), "close_radius"),
    "close_radius inf": (lambda n: _seg_field(n, 1, close_radius=float("inf")), "close_radius"),
    "range min >= max": (lambda n: _arr(n, "range", 4, -1.0), "range"),
    "range nan": (lambda n: _arr(n, "range", 0, float("nan")), "range"),
    "range inf": (lambda n: _arr(n, "range", 5, float("inf")), "range"),
    "null count": (lambda n: _args(n, null=False, count=None), "count"),
    "null src": (lambda n: _args(n, null=False, src=None), "src"),
    "null dst": (lambda n: _args(n, null=False, dst=None), "src, dst"),
    "null workspace": (lambda n: _args(n, null=False, workspace=None), "workspace"),
    "workspace too small": (lambda n: _args(n, null=False, workspace_bytes=3), "workspace below"),
    "all null": (lambda n: _args(n), "count"),
}


@pytest.mark.parametrize("case", sorted(REJECTS))
def test_pts_prepare_rejects(case):
    native, L = _lib()
    make, text = REJECTS[case]
    a = make(native)
    rc = L.cmt_pts_prepare(ctypes.byref(a), None)
    msg = L.cmt_last_error().decode()
    assert rc == 1001, f"{case}: status {rc}"   # CMT_EINVAL
    assert text in msg, f"{case}: {msg!r}"
    assert L.cmt_pts_prepare(None, None) == 1001
