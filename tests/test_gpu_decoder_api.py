"""PETRTransformerDecoder through the reference's module API
(petr_transformer.py:347-371: forward(query, key, value, query_pos=, key_pos=),
sequence-first tensors) on the fused path: a zero target equals the frame's
path (run_rows) bit for bit, a non-zero target is held to the CPU restatement
(oracle/cmt_oracle.py decoder) by tests/test_gpu_head.py's rule, and the layer
walk queues exactly the launches it is documented to queue."""
import pytest
import torch

from projects.mmdet3d_plugin.runtime import options

pytestmark = pytest.mark.gpu

B, NQ, NK, L, C = 2, 37, 96, 2, 256   # a ragged last row block (74 rows), B > 1, a layer with a next layer + the last


@pytest.fixture(scope="module")
def case():
    """The decoder of a two-layer synthetic head, seeded sequence-first inputs and the oracle's
    outputs for them (fp16 / fp32 cross-attention core), computed once."""
    from oracle import cmt_oracle as O
    from projects.mmdet3d_plugin import synthetic as S
    head, _, _ = S.build_synthetic_head("cmt_fusion_nus", seed=3, num_query=NQ, num_layers=L,
                                        grid_size=[256, 256, 40])
    g = torch.Generator().manual_seed(1)
    query, query_pos = torch.randn(NQ, B, C, generator=g), torch.randn(NQ, B, C, generator=g)
    key, key_pos = torch.randn(NK, B, C, generator=g), torch.randn(NK, B, C, generator=g)
    sd = S.head_state_dict(head)
    with torch.no_grad():
        refs = {c: O.decoder(query, key, query_pos, key_pos, sd, "transformer.decoder", L, cross_core=c)
                for c in ("fp16", "fp32")}
    return dict(head=head, query=query, query_pos=query_pos, key=key, key_pos=key_pos, refs=refs)


def _on(case, dev, prec, chain, fn):
    """fn(decoder, inputs on dev) under a precision policy and a chain setting."""
    from projects.mmdet3d_plugin import set_precision
    head = case["head"].to(dev)
    t = {k: case[k].to(dev) for k in ("query", "query_pos", "key", "key_pos")}
    set_precision(prec)
    try:
        with torch.no_grad(), options(chain=chain):
            out = fn(head.transformer.decoder, t)
        torch.cuda.synchronize()
    finally:
        set_precision("ref")
        head.cpu()
    return out


def _rows(x):
    """Sequence-first [N, B, C] -> batch-major fp32 rows [B * N, C]."""
    return x.transpose(0, 1).reshape(-1, x.shape[-1]).contiguous().float()


def _module_api(dec, t, query):
    return dec(query, t["key"], None, query_pos=t["query_pos"], key_pos=t["key_pos"])


def _frame_path(dec, t):
    out = dec.run_rows(_rows(t["key"]), _rows(t["key_pos"]), _rows(t["query_pos"]), B=B, Nk=NK, Nq=NQ, post_flags=0)
    return out.view(L, B, NQ, C).transpose(1, 2)


@pytest.mark.parametrize("chain", [True, False])
@pytest.mark.parametrize("prec", ["ref", "bf16", "fp16"])
def test_zero_target_module_api_equals_frame_path(dev, case, prec, chain):
    """A zero residual added in fp32 changes no value and add_cast of zeros equals add_cast(None),
    so the module API with a zero query is the frame's zero-target run_rows, bit for bit."""
    a, b = _on(case, dev, prec, chain, lambda dec, t: (_module_api(dec, t, torch.zeros_like(t["query_pos"])).clone(),
                                                       _frame_path(dec, t).clone()))
    assert a.shape == b.shape == (L, NQ, B, C) and torch.isfinite(b).all()
    assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("chain", [True, False])
def test_nonzero_target_matches_oracle(dev, case, parity_log, chain):
    """A non-zero target (layer 0's residual is the query) on the raw decoder outputs, by
    test_gpu_head.py's rule: 'ref' vs the fp16-core oracle max <= max(2.5e-3, 1.5 floor), mean <=
    max(5e-4, 1.5 floor_mean); 'ref' vs exact fp32 max <= max(5e-3, 1.5 floor); bf16 vs fp32 <=
    2.5e-2 of max |ref| (floor: the oracle's fp16 core against its fp32 core, 3.4e-4 .. 3.8e-4 max
    / 5.2e-5 mean on these inputs depending on the host's BLAS; outputs reach 5.07)."""
    r16, r32 = case["refs"]["fp16"].double(), case["refs"]["fp32"].double()
    floor, floor_mean = (r16 - r32).abs().max().item(), (r16 - r32).abs().mean().item()
    got = _on(case, dev, "ref", chain, lambda dec, t: _module_api(dec, t, t["query"]).clone()).cpu().double()
    gotb = _on(case, dev, "bf16", chain, lambda dec, t: _module_api(dec, t, t["query"]).clone()).cpu().double()
    e16, m16 = (got - r16).abs().max().item(), (got - r16).abs().mean().item()
    e32 = (got - r32).abs().max().item()
    eb = (gotb - r32).abs().max().item() / r32.abs().max().item()
    print(f"oracle fp16-core floor: max {floor:.2e} mean {floor_mean:.2e}; 'ref' vs fp16 core: max {e16:.2e} mean "
          f"{m16:.2e}; vs fp32: max {e32:.2e}; bf16 vs fp32: {eb:.2e} of max |ref| {r32.abs().max().item():.2f}")
    parity_log.append(f"decoder module API, non-zero target (chain={chain}, {B} x {NQ} queries, {NK} keys, {L} "
                      f"layers): 'ref' vs fp16-core oracle max {e16:.2e} mean {m16:.2e}, vs fp32 max {e32:.2e} "
                      f"(floor {floor:.2e}); bf16 vs fp32 {eb:.2e} of scale (bound 2.5e-2)")
    assert e16 <= max(2.5e-3, 1.5 * floor), e16
    assert m16 <= max(5e-4, 1.5 * floor_mean), m16
    assert e32 <= max(5e-3, 1.5 * floor), e32
    assert eb <= 2.5e-2, eb


SPIED = ("add_cast", "kv_proj", "gemm", "attention", "chain", "layernorm_ex", "split_rows", "cast")
CHAIN_SEQ = ["add_cast", "kv_proj", "add_cast", "gemm",
             "attention", "chain0", "attention", "chain1", "chain2",
             "attention", "chain0", "attention", "chain1", "chain2"]
SEP_SEQ = ["add_cast", "kv_proj", "add_cast",
           "gemm", "attention", "gemm", "layernorm_ex", "gemm", "attention", "gemm", "layernorm_ex", "gemm", "gemm",
           "layernorm_ex",
           "gemm", "attention", "gemm", "layernorm_ex", "gemm", "attention", "gemm", "layernorm_ex", "gemm", "gemm",
           "layernorm_ex"]


def _launches(case, dev, chain, fn):
    """The native launches fn queues, in order (chain launches with their kind)."""
    from projects.mmdet3d_plugin import native
    seen, real = [], {n: getattr(native, n) for n in SPIED}

    def spy(name):
        def call(*a, **kw):
            seen.append(name + str(a[0]) if name == "chain" else name)
            return real[name](*a, **kw)
        return call
    for n in SPIED:
        setattr(native, n, spy(n))
    try:
        _on(case, dev, "ref", chain, fn)
    finally:
        for n in SPIED:
            setattr(native, n, real[n])
    return seen


@pytest.mark.parametrize("target", ["zero", "nonzero"])
def test_launch_sequence_chain(dev, case, target):
    """'ref' policy, chain path, run_rows without a state or K/V operands: the memory-side
    add_cast and K/V projection, the target's add_cast and layer 0's in_proj GEMM, then per layer
    self-attention, chain A, cross-attention, chains B1 and B2 (B2 runs the next layer's in_proj).
    A non-zero target queues the same launches."""
    fn = _frame_path if target == "zero" else (lambda dec, t: _module_api(dec, t, t["query"]))
    assert _launches(case, dev, True, fn) == CHAIN_SEQ


@pytest.mark.parametrize("target", ["zero", "nonzero"])
def test_launch_sequence_separate(dev, case, target):
    """options(chain=False): the same walk as separate launches, recorded with this spy before
    the chain and separate-launch loops were merged."""
    fn = _frame_path if target == "zero" else (lambda dec, t: _module_api(dec, t, t["query"]))
    assert _launches(case, dev, False, fn) == SEP_SEQ
