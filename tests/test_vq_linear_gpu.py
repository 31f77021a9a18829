"""The per-row linear map on the GPU: functional.linear_rows / linear_rows_backward (vqvae_linear_rows_*_f32) and training.LinearRows
against the CPU restatement tests/vq_linear_ref.py, whose arithmetic is the header of vqvae_amd/csrc/vq_linear.hip.  Every operation of
the contract is a correctly rounded IEEE operation in a fixed order, so every output is compared bit for bit, on every element (NaNs by
position): in both layouts, on the 16-byte path and with every tensor offset by 4 bytes, in two runs and in a graph replay."""
import numpy as np
import pytest
import torch

from tests import vq_linear_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a, offset=False):
    """a numpy array on the device; offset: one float into a larger buffer, so that no 16-byte access path takes it"""
    t = torch.from_numpy(np.array(a, order="C"))               # (a copy: the cases' arrays are read-only)
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _layout(rows, B, H, W, rowmajor, offset=False):
    z = np.ascontiguousarray(rows).reshape(B, H, W, rows.shape[1])
    return _dev(z if rowmajor else z.transpose(0, 3, 1, 2), offset)


def _rows(t, rowmajor):
    t = t.detach().cpu()
    t = t if rowmajor else t.permute(0, 2, 3, 1)
    return np.ascontiguousarray(t.contiguous().numpy().reshape(-1, t.shape[-1]))


def _check(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions"
    diff = got.view(np.uint32)[~gn] != want.view(np.uint32)[~wn]
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits"


def _check_all(outs, case, rowmajor, what):
    _, _, _, _, y, gx, gw, gb = R.expected(case)
    _check(_rows(outs[0], rowmajor), y, f"{what}: y")
    _check(_rows(outs[1], rowmajor), gx, f"{what}: grad_x")
    _check(outs[2].cpu().numpy(), gw, f"{what}: grad_w")
    _check(outs[3].cpu().numpy(), gb, f"{what}: grad_b")


def _inputs(case, rowmajor, offset=False):
    B, H, W, Cin, Cout = case
    x, gy, w, b = R.expected(case)[:4]
    return _layout(x, B, H, W, rowmajor, offset), _layout(gy, B, H, W, rowmajor, offset), _dev(w, offset), _dev(b, offset)


def _chain(xt, gt, wt, bt, rowmajor):
    from vqvae_amd import functional as F
    return (F.linear_rows(xt, wt, bt, rowmajor=rowmajor),) + F.linear_rows_backward(xt, gt, wt, rowmajor=rowmajor)


@pytest.mark.parametrize("case", R.GPU_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bits_in_both_layouts_on_both_paths_and_in_two_runs(case):
    for rowmajor in (True, False):
        for offset in (False, True):
            t = _inputs(case, rowmajor, offset)
            for run in range(2 if not offset else 1):
                outs = _chain(*t, rowmajor)
                torch.cuda.synchronize()
                assert outs[0].shape[0] == case[0] and outs[1].shape == t[0].shape
                _check_all(outs, case, rowmajor, f"rowmajor={rowmajor} offset={offset} run {run}")


@pytest.mark.parametrize("rowmajor", [True, False])
@pytest.mark.parametrize("case", R.GPU_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bits_in_a_graph_replay(case, rowmajor):
    """forward and backward are one chain of launches on one stream: captured, and replayed on new inputs with other values left in
    the outputs between the replays"""
    real = _inputs(case, rowmajor)
    xs, gs = torch.zeros_like(real[0]), torch.zeros_like(real[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _chain(xs, gs, real[2], real[3], rowmajor)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _chain(xs, gs, real[2], real[3], rowmajor)
    xs.copy_(real[0])
    gs.copy_(real[1])
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _check_all(outs, case, rowmajor, f"replay {i}")
        for o in outs:
            o.fill_(7.0)


def test_a_two_dimensional_tensor_is_taken_as_rows():
    from vqvae_amd import functional as F
    case = (5, 9, 9, 64, 8)
    x, gy, w, b, y, gx, gw, gb = R.expected(case)
    xt, gt, wt, bt = _dev(x), _dev(gy), _dev(w), _dev(b)
    got = F.linear_rows(xt, wt, bt)
    assert got.shape == (405, 8)
    _check(got.cpu().numpy(), y, "y of (N, Cin) rows")
    out = F.linear_rows_backward(xt, gt, wt)
    _check(out[0].cpu().numpy(), gx, "grad_x")
    _check(out[1].cpu().numpy(), gw, "grad_w")
    _check(out[2].cpu().numpy(), gb, "grad_b")


@pytest.mark.parametrize("rowmajor", [True, False])
def test_every_combination_of_wanted_gradients(rowmajor):
    from vqvae_amd import functional as F
    case = (4, 8, 8, 65, 33)
    xt, gt, wt, bt = _inputs(case, rowmajor)
    _, _, _, _, _, gx, gw, gb = R.expected(case)
    ws = F.linear_rows_backward_workspace(256, 65, 33, DEV)
    for want in [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False) if a or b or c]:
        out = F.linear_rows_backward(xt, gt, wt, rowmajor=rowmajor, want=want, workspace=ws if want[1] else None)
        assert [o is not None for o in out] == list(want)
        if want[0]:
            _check(_rows(out[0], rowmajor), gx, f"{want}: grad_x")
        if want[1]:
            _check(out[1].cpu().numpy(), gw, f"{want}: grad_w")
        if want[2]:
            _check(out[2].cpu().numpy(), gb, f"{want}: grad_b")
    with pytest.raises(ValueError):
        F.linear_rows_backward(xt, gt, wt, rowmajor=rowmajor, want=(False, False, False))


def test_argument_errors_come_back_without_a_launch():
    from vqvae_amd import _lib, functional as F
    L = _lib.load()
    case = (2, 7, 7, 6, 5)
    xt, gt, wt, bt = _inputs(case, True)
    st = torch.cuda.current_stream().cuda_stream
    y = torch.full((2, 7, 7, 5), 7.0, device=DEV)
    gx, gw, gb = torch.full_like(xt, 7.0), torch.full_like(wt, 7.0), torch.full_like(bt, 7.0)
    ws = F.linear_rows_backward_workspace(98, 6, 5, DEV)
    bw = lambda gx_, gw_, gb_, ws_, n: L.vqvae_linear_rows_backward_f32(xt.data_ptr(), gt.data_ptr(), wt.data_ptr(), 2, 6, 7, 7, 5, 1,
                                                                       gx_, gw_, gb_, ws_, n, st)
    assert bw(None, None, None, ws.data_ptr(), ws.numel()) == -1                                   # no gradient asked for
    assert bw(gx.data_ptr(), gw.data_ptr(), None, None, 0) == -4                                   # grad_w without a workspace
    assert bw(gx.data_ptr(), None, gb.data_ptr(), ws.data_ptr(), ws.numel() - 8) == -4             # the workspace too small
    assert bw(xt.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws.numel()) == -3        # grad_x on x
    assert bw(gx.data_ptr(), wt.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws.numel()) == -3        # grad_w on w
    assert bw(gx.data_ptr(), gw.data_ptr(), gb.data_ptr(), gt.data_ptr(), ws.numel()) == -3        # the workspace on grad_y
    assert L.vqvae_linear_rows_forward_f32(xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), 2, 6, 7, 7, 5, 1, xt.data_ptr(), st) == -3
    assert L.vqvae_linear_rows_forward_f32(xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), 2, 6, 7, 7, 257, 1, y.data_ptr(), st) == -3
    with pytest.raises(_lib.VqvaeHipError):
        F.linear_rows(torch.zeros(1, 2, 2, 4, device=DEV), torch.zeros(257, 4, device=DEV), torch.zeros(257, device=DEV), rowmajor=True)
    with pytest.raises(_lib.VqvaeHipError):
        F.linear_rows_backward(xt, gt, wt, rowmajor=True, workspace=ws[:8])
    with pytest.raises(ValueError):
        F.linear_rows(xt, wt.t().contiguous(), bt, rowmajor=True)
    torch.cuda.synchronize()
    for t in (y, gx, gw, gb):
        assert bool((t == 7.0).all())                                                              # nothing was launched
    # ... and grad_x alone needs no workspace
    out = L.vqvae_linear_rows_backward_f32(xt.data_ptr(), gt.data_ptr(), wt.data_ptr(), 2, 6, 7, 7, 5, 1, gx.data_ptr(), None, None, None, 0, st)
    assert out == 0
    _check(_rows(gx, True), R.expected(case)[5], "grad_x alone")


@pytest.mark.parametrize("rowmajor", [True, False])
def test_linear_rows_under_autograd_asks_only_for_what_is_needed(rowmajor, monkeypatch):
    from vqvae_amd import functional as F, training as T
    case = (5, 9, 9, 64, 8)
    xt, gt, wt, bt = _inputs(case, rowmajor)
    _, _, _, _, y, gx, gw, gb = R.expected(case)
    asked = []
    real = F.linear_rows_backward
    monkeypatch.setattr(F, "linear_rows_backward", lambda *a, **k: (asked.append(k["want"]), real(*a, **k))[1])
    for need in [(True, True, True), (True, False, False), (False, True, True), (False, False, True)]:
        x_, w_, b_ = (t.clone().requires_grad_(n) for t, n in zip((xt, wt, bt), need))
        out = T.LinearRows.apply(x_, w_, b_, rowmajor)
        _check(_rows(out, rowmajor), y, "y")
        out.backward(gt)
        assert asked[-1] == need
        for t, n, want, rows in ((x_, need[0], gx, True), (w_, need[1], gw, False), (b_, need[2], gb, False)):
            assert (t.grad is not None) == n
            if n:
                _check(_rows(t.grad, rowmajor) if rows else t.grad.cpu().numpy(), want, f"{need}")
