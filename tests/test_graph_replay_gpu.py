"""Graph replay of every captured path against the bits of an eager call (tests/graph_replay.py builds the inputs; the CPU file
checks their properties).

Every capture is one linear chain on one private stream after an eager warm-up on that stream.  Before every replay every static
output is overwritten with 0xFF bytes; after it every output must equal, bit for bit, an eager call on fresh tensors holding the
same input.  A replay launches the kernels of the capture with the launch shapes of the capture: there is no tolerance.

  1  the stand-alone quantizer on each of its kernel routes, with the prepare kernels and their clears inside the graph and with a
     caller's prepared workspace, over input states that fill disjoint parts of the histogram;
  2  forward / encode / decode_indices of the whole-path entries on each of their routes, over images whose per-image magnitude moves
     up, down and through zero between replays;
  3  the captured training step (zero_grad, forward, losses, backward, HIP Adam) against an eagerly stepped twin;
  4  eager evaluations between replays of the step see the replayed weights (GraphedStep, or a raw graph and invalidate_caches())."""
import faulthandler

import numpy as np
import pytest
import torch

from tests import graph_replay as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _limit(fn):
    """the test's own time limit: a replay that hangs ends the process"""
    import functools

    @functools.wraps(fn)
    def run(*a, **k):
        faulthandler.dump_traceback_later(120, exit=True)
        try:
            return fn(*a, **k)
        finally:
            faulthandler.cancel_dump_traceback_later()
    return run


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the stand-alone quantizer -------------------------------------------------------------------------------------------------
_VQ_EAGER = {}


def _vq_eager(case):
    """the eager outputs of the four states, on fresh tensors and a workspace of their own: computed once per case"""
    from vqvae_amd import functional as F
    if case not in _VQ_EAGER:
        c = G.VQ_CASES[case]
        cb = _t(G.vq_codebook(case))
        outs = []
        for rows in G.vq_states(case)[:3]:
            out = F.vq_forward(_t(G.vq_layout(case, rows)), cb, G.BETA, rowmajor=c["rowmajor"], bf16_filter=c["bf16"])
            outs.append([t.clone() for t in out])
        torch.cuda.synchronize()
        _VQ_EAGER[case] = outs + [outs[0]]
    return _VQ_EAGER[case]


@pytest.mark.parametrize("own_workspace", [False, True], ids=["prepare_in_graph", "prepared_workspace"])
@pytest.mark.parametrize("case", sorted(G.VQ_CASES))
@_limit
def test_quantizer_replay_on_every_route(case, own_workspace):
    from vqvae_amd import _lib, functional as F
    c = G.VQ_CASES[case]
    K, D = c["K"], c["D"]
    n = G.B_VQ * c["H"] * c["W"]
    # the case sits on its route
    assert _lib.vq_kernel_name(K, D, G.vq_flags(case)) == c["name"]
    if case == "filter_nchw_7x7":
        # (vq_kernel_name answers for 8x8 maps; at HW = 49 the tracker does not run, and the two-sweep filter kernel is what a D = 64
        # codebook of this size falls to)
        assert _lib.vq_launch_form(n, K, D, c["H"] * c["W"], 0x0) is None and _lib.vq_launch_form(n, K, D, 64, 0x0) is not None
        assert _lib.vq_kernel_name(K, D, 0x8) == "vq_filter_kernel_d64"
    states = G.vq_states(case)
    eager = _vq_eager(case)
    cb = _t(G.vq_codebook(case))
    static_z = _t(G.vq_layout(case, states[0]))
    ws = None
    if own_workspace:
        ws = F.vq_workspace(K, D, DEV)
        F.vq_forward(static_z, cb, G.BETA, rowmajor=c["rowmajor"], bf16_filter=c["bf16"], workspace=ws)      # prepares the images
        torch.cuda.synchronize()

    def fn():
        return F.vq_forward(static_z, cb, G.BETA, rowmajor=c["rowmajor"], bf16_filter=c["bf16"], workspace=ws,
                            prepared=own_workspace)

    with torch.no_grad():
        cap = G.Captured(fn, DEV)
    names = ("loss", "z_q", "perplexity", "idx", "hist")
    for r, (rows, want) in enumerate(zip(states, eager)):
        static_z.copy_(_t(G.vq_layout(case, rows)))
        G.poison(cap.out[0], *cap.out[1:])               # (loss and perplexity are views of one tensor: both are poisoned)
        out = cap.replay()
        torch.cuda.synchronize()
        idx, hist = out[3], out[4]
        # independent of any eager call: the histogram is the indices', and nothing of another replay is in it
        assert int(idx.min()) >= 0 and int(idx.max()) < K, f"state {r}: an index outside [0, K)"
        assert torch.equal(hist.to(torch.int64), torch.bincount(idx.view(-1), minlength=K)), f"state {r}: hist != bincount(idx)"
        assert int(hist.sum()) == n
        for name, a, b in zip(names, out, want):
            assert G.same_bits(a, b), f"state {r}: {name} differs from the eager call in {G.differing(a, b)} of {a.numel()} elements"
    # the states did what they are for on the device too: b and c used disjoint code sets
    assert not (set(eager[1][3].view(-1).tolist()) & set(eager[2][3].view(-1).tolist()))


# ---- 2. the whole-path entries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.MODEL_CASES))
@_limit
def test_whole_path_entries_replay_on_every_route(case):
    from vqvae_amd import conv
    from vqvae_amd.graph import GraphedForward
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    c = G.MODEL_CASES[case]
    B, HW, K = c["B"], c["HW"], c["dims"][3]
    assert VQVAE.FORWARD_PARTS == 1
    torch.manual_seed(11)
    m = VQVAE(*c["dims"], G.BETA).to(DEV).eval()
    xs = [_t(x) for x in G.model_images(case)]
    ids = [_t(i) for i in G.model_indices(case)]
    h = HW // 4
    with torch.no_grad():
        e_fwd = [[t.clone() for t in m(x)] for x in xs[:4]]
        e_enc = [m.encode(x).clone() for x in xs[:4]]
        e_dec = [m.decode_indices(i, B, h, h, validate=False).clone() for i in ids[:4]]
    torch.cuda.synchronize()
    for e in (e_fwd, e_enc, e_dec):
        e.append(e[0])
    assert not (set(ids[0].view(-1).tolist()) & set(ids[1].view(-1).tolist()))
    # the images' magnitudes reach the outputs: the all-zero image reconstructs to something else than the unit-scale one
    assert not G.same_bits(e_fwd[0][1][0], e_fwd[3][1][0])

    g_fwd = GraphedForward(m, xs[0])
    static_x = xs[0].clone()
    static_i = ids[0].clone()
    with torch.no_grad():
        g_enc = G.Captured(lambda: m.encode(static_x), DEV)
        g_dec = G.Captured(lambda: m.decode_indices(static_i, B, h, h, validate=False), DEV)
    for r in range(G.N_REPLAYS):
        G.poison(g_fwd.static_out[0], g_fwd.static_out[1], g_fwd.static_out[2])
        out = g_fwd(xs[r])
        torch.cuda.synchronize()
        for name, a, b in zip(("embedding_loss", "x_hat", "perplexity"), out, e_fwd[r]):
            assert G.same_bits(a, b), f"forward, replay {r}: {name} differs in {G.differing(a, b)} of {a.numel()} elements"
        static_x.copy_(xs[r])
        G.poison(g_enc.out)
        idx = g_enc.replay()
        torch.cuda.synchronize()
        assert G.same_bits(idx, e_enc[r]), f"encode, replay {r}: {G.differing(idx, e_enc[r])} of {idx.numel()} indices differ"
        assert int(idx.min()) >= 0 and int(idx.max()) < K
        static_i.copy_(ids[r])
        G.poison(g_dec.out)
        x_hat = g_dec.replay()
        torch.cuda.synchronize()
        assert G.same_bits(x_hat, e_dec[r]), f"decode_indices, replay {r}: {G.differing(x_hat, e_dec[r])} of {x_hat.numel()} differ"


# ---- 3. the captured training step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.STEP_CASES))
@_limit
def test_training_step_replay_equals_eager_twin(case):
    a, oa, b, ob = G.make_twins(case, DEV)
    xs = [_t(x) for x in G.step_images(case, 4)]
    xa, xb = xs[0].clone(), xs[0].clone()
    step_a, step_b = G.make_step(a, oa, xa), G.make_step(b, ob, xb)
    for _ in range(G.N_WARMUP):
        step_a()
    cap = G.Captured(step_b, DEV, warmup=G.N_WARMUP)
    torch.cuda.synchronize()
    G.assert_same_state(a, oa, b, ob, "after the warm-up")
    for r, x in enumerate(xs[1:]):
        xa.copy_(x)
        st_a = step_a()
        xb.copy_(x)
        # the static outputs and the gradients the step zeroes and accumulates into: a kernel that fails to write shows
        G.poison(cap.out, *[p.grad for p in b.parameters() if p.grad is not None])
        st_b = cap.replay()
        torch.cuda.synchronize()
        assert G.same_bits(st_a, st_b), f"replay {r}: stats {st_b.tolist()} != eager {st_a.tolist()}"
        assert bool(torch.isfinite(st_a).all())
        G.assert_same_state(a, oa, b, ob, f"replay {r}")
    steps = {float(s["step"]) for s in ob.state.values()}
    assert steps == {float(G.N_WARMUP + 3)}
    if G.STEP_CASES[case].get("max_grad_norm"):
        assert G.same_bits(oa.last_grad_norm, ob.last_grad_norm) and float(oa.last_grad_norm) > G.STEP_CASES[case]["max_grad_norm"]


# ---- 4. eager calls after replays see the replayed weights -------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["graphed_step", "raw_graph_then_invalidate_caches"])
@pytest.mark.parametrize("case", ["plain", "ema"])
@_limit
def test_eager_evaluation_between_replays_sees_the_replayed_weights(case, how):
    from vqvae_amd.graph import GraphedStep
    a, oa, b, ob = G.make_twins(case, DEV, seed=1)
    xs = [_t(x) for x in G.step_images(case, 5)]
    x_eval = xs[4]
    xa = xs[0].clone()
    step_a = G.make_step(a, oa, xa)
    for _ in range(G.N_WARMUP):
        step_a()
    if how == "graphed_step":
        def step(x):
            return G.make_step(b, ob, x)()
        g = GraphedStep(b, step, xs[0], warmup=G.N_WARMUP)

        def replay(x):
            return g(x)
    else:
        xb = xs[0].clone()
        cap = G.Captured(G.make_step(b, ob, xb), DEV, warmup=G.N_WARMUP)

        def replay(x):
            xb.copy_(x)
            return cap.replay()
    k = 0
    evals = []
    for name in ("A", "B"):
        for _ in range(2):
            x = xs[k % 4]
            k += 1
            xa.copy_(x)
            st_a = step_a()
            st_b = replay(x)
            torch.cuda.synchronize()
            assert G.same_bits(st_a, st_b)
        if how != "graphed_step":
            b.invalidate_caches()                       # a raw replay leaves `_version` alone: the caller's duty
        ea, eb = G.evaluate(a, x_eval), G.evaluate(b, x_eval)
        torch.cuda.synchronize()
        evals.append(ea)
        for what, ta, tb in zip(("embedding_loss", "x_hat", "perplexity", "encode", "decode_indices(encode)"), ea, eb):
            assert G.same_bits(ta, tb), (f"evaluation {name} after {k} replays: {what} differs from the eagerly trained twin in "
                                         f"{G.differing(ta, tb)} of {ta.numel()} elements")
        G.assert_same_state(a, oa, b, ob, f"evaluation {name}")
    # the weights moved between the two evaluations far enough to show: a stale image would not have gone unnoticed
    assert not G.same_bits(evals[0][1], evals[1][1])
