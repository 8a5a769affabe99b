"""cmt_lsap's argument checks and the device_assign option, without a device:
every check below runs before any launch (include/cmt_hip.h cmt_lsap)."""
import ctypes


def _args(P=3, max_nq=900, max_ngt=100):
    """A cmt_lsap_args whose pointers are non-null but never dereferenced (the checks under
    test return before a launch)."""
    from projects.mmdet3d_plugin import native
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    a = native.LsapArgs()
    a.P, a.max_nq, a.max_ngt = P, max_nq, max_ngt
    a.cost, a.cost_elems, a.desc = ptr, 16, ptr
    a.match_q, a.ld_q, a.match_g, a.ld_g = ptr, max_ngt, ptr, max_nq
    a.status, a.workspace, a.workspace_bytes = ptr, ptr, 0
    a._keep = buf
    return a


def test_lsap_struct_size_matches_the_library():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    assert L.cmt_lsap_args_size() == ctypes.sizeof(native.LsapArgs)
    assert native.STRUCTS["lsap"] is native.LsapArgs
    assert L.cmt_abi_version() == 25          # the new symbols are additive


def test_lsap_rejects_no_problems_and_null_pointers():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    for P in (0, -1):
        a = _args(P=P)
        assert L.cmt_lsap(ctypes.byref(a), None) == 1001
        assert b"cmt_lsap" in L.cmt_last_error() and b"P" in L.cmt_last_error()
    for field in ("cost", "desc", "match_q", "status", "workspace"):
        a = _args()
        setattr(a, field, None)
        assert L.cmt_lsap(ctypes.byref(a), None) == 1001, field
        assert b"non-null" in L.cmt_last_error(), field
    assert L.cmt_lsap(None, None) == 1001
    a = _args()
    a.ld_q = a.max_ngt - 1                    # an output row shorter than the largest problem
    assert L.cmt_lsap(ctypes.byref(a), None) == 1001


def test_lsap_reports_oversize_problems_as_unsupported():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    for nq, ngt in ((2049, 10), (10, 2049), (600, 513), (513, 2048)):
        a = _args(max_nq=nq, max_ngt=ngt)
        assert L.cmt_lsap(ctypes.byref(a), None) == 1002, (nq, ngt)
        assert b"2048" in L.cmt_last_error() and b"512" in L.cmt_last_error()
    # inside the limits the next check is the workspace size (still before any launch)
    for nq, ngt in ((2048, 512), (512, 2048), (900, 100)):
        a = _args(max_nq=nq, max_ngt=ngt)
        assert L.cmt_lsap(ctypes.byref(a), None) == 1003, (nq, ngt)


def test_lsap_workspace_bytes_positive_and_monotone():
    from projects.mmdet3d_plugin import native
    L = native.lib()
    base = L.cmt_lsap_workspace_bytes(4, 900, 100)
    assert base >= 4 * 900 * 100 * 4          # every matrix fits, as fp32
    assert L.cmt_lsap_workspace_bytes(1, 1, 1) > 0
    for more in ((5, 900, 100), (4, 901, 100), (4, 900, 101), (8, 2048, 512)):
        assert L.cmt_lsap_workspace_bytes(*more) >= base, more
    assert L.cmt_lsap_workspace_bytes(8, 2048, 512) > base
    prev = 0
    for P in range(1, 6):
        cur = L.cmt_lsap_workspace_bytes(P, 64, 8)
        assert cur >= prev and cur > 0
        prev = cur


def test_lsap_binding_refuses_cpu_tensors():
    import pytest
    import torch
    from projects.mmdet3d_plugin import native_train as T
    desc = torch.tensor([[0, 4, 2, 2]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        T.lsap(torch.zeros(8), desc, max_nq=4, max_ngt=2)


def test_device_assign_option_is_off_by_default():
    import os
    from projects.mmdet3d_plugin import runtime
    assert "device_assign" in runtime.Options.__dataclass_fields__
    assert runtime.Options.__dataclass_fields__["device_assign"].default is False
    # read once from the environment at import: on only with CMT_DEVICE_ASSIGN=1
    assert runtime.OPTIONS.device_assign is (os.environ.get("CMT_DEVICE_ASSIGN", "0") == "1")
    before = runtime.OPTIONS.device_assign
    with runtime.options(device_assign=True) as o:
        assert o.device_assign is True
    assert runtime.OPTIONS.device_assign is before
