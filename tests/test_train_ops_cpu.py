"""Host-side pieces of the training ops that need no GPU: the kernel-3 tap gather of the task
heads' grouped convs (train_ops.taps3) against the pad + three slices + cat it replaces, values
and gradients in float64."""
import torch
import torch.nn.functional as F


def test_taps3_matches_pad_slices():
    from projects.mmdet3d_plugin.models.utils import train_ops as ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(6, 2, 37, 64, dtype=torch.float64, generator=g, requires_grad=True)
    dy = torch.randn(6, 2, 37, 192, dtype=torch.float64, generator=g)
    y = ops.taps3(x)
    y.backward(dy)
    got = x.grad.clone()
    x.grad = None
    n = x.shape[-2]
    xp = F.pad(x, (0, 0, 1, 1))
    want = torch.cat([xp[..., 0:n, :], xp[..., 1:n + 1, :], xp[..., 2:n + 2, :]], -1)
    want.backward(dy)
    assert torch.equal(y, want)
    assert (got - x.grad).abs().max().item() < 1e-12


def test_det_loss_grad_buffers_keep_the_input_row_stride():
    """native_train._grad_like_rows: cmt_det_loss addresses an input and its gradient with ONE row
    stride (dlogits[r * ld_logits + c]), so the gradient buffer of a column slice must span
    R * ld elements with the slice's row stride -- zeros_like of the slice is dense (R * width)
    and the kernel would write past it."""
    from projects.mmdet3d_plugin import native_train as T
    parent = torch.randn(6, 20)
    for x in (parent[:, :10], parent[:, 3:13], parent, torch.randn(6, 10), parent[:1, 3:13], parent[:0, :10]):
        g = T._grad_like_rows(x)
        R, ld = x.shape[0], x.stride(0)
        assert g.shape == x.shape and g.dtype == x.dtype
        if R > 1:
            assert g.stride(0) == ld
        assert g.shape[1] <= 1 or g.stride(1) == 1
        # every element the kernel may address, g[r * ld + c] for r < R, c < width, is in the storage
        elems = g.untyped_storage().nbytes() // g.element_size() - g.storage_offset()
        assert R == 0 or elems >= (R - 1) * ld + x.shape[1]
        if ld != x.shape[1] and R > 1:
            assert elems >= R * ld
            assert float(g._base.abs().sum()) == 0.0      # the gap columns start as zeros
    for bad in (parent.t(), parent[:, ::2], torch.randn(6)):
        try:
            T._grad_like_rows(bad)
        except RuntimeError:
            continue
        raise AssertionError("a transposed / column-strided / 1-D input must be rejected")
