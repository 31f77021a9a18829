"""The split EMA codebook update without a GPU: the fp64 restatement (tests/vq_ema_merge_ref.py) against the one-shot restatement of
tests/vq_ema_ref.py, the restart rule across shards, the kernels' own text on the host under the sanitizers, the C ABI's four entries
(declared, bound, argument errors before any launch, ABI still 9), the front ends' refusal of CPU tensors, the constructor rules,
the unchanged default model, the train tool's options and the two collectives on a 2-rank gloo group."""
import os
import re
import shutil
import socket
import struct

import numpy as np
import pytest
import torch

from tests import vq_ema_merge_ref as M
from tests import vq_ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _draw(N, D, K, seed, skew=False):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, D, generator=g)
    idx = torch.randint(0, K, (N,), generator=g)
    if skew:
        idx[torch.rand(N, generator=g) < 0.8] = 0
    cs = torch.rand(K, generator=g) * 5
    w = torch.randn(K, D, generator=g)
    return z, idx, cs, w


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,D,K", [(40, 5, 7), (1, 1, 1), (300, 3, 16)])
def test_one_shard_is_the_one_shot_update(N, D, K):
    z, idx, cs, w = _draw(N, D, K, N + K)
    u = torch.rand(K, generator=torch.Generator().manual_seed(3))
    for thr in (None, 2.0):
        st = M.stats(z, idx, K, u if thr is not None else None)[None]
        got = M.apply(st, cs, w, 0.9, 1e-5, thr, torch.zeros(K) if thr is not None else None)
        for ref in (R.ema_update(z, idx, cs, w, 0.9, 1e-5, thr, u), R.ema_update_loop(z, idx, cs, w, 0.9, 1e-5, thr, u)):
            for k in ("N", "m", "e"):
                torch.testing.assert_close(got[k], ref[k], rtol=1e-13, atol=1e-13)
            assert float(got["n"]) == pytest.approx(float(ref["n"]), rel=1e-14)
        assert torch.equal(got["N"], R.ema_update(z, idx, cs, w, 0.9, 1e-5, thr, u)["N"])          # counts are exact


@pytest.mark.parametrize("sizes", [(100, 37, 163), (1, 50, 20, 9, 70, 100, 49, 1)])
def test_merged_shards_agree_with_the_one_shot_update(sizes):
    """N, m, e from 3 and from 8 shards against the whole batch at once: the only difference is the order of the fp64 sums, so the
    counts are exact and m, e agree to fp64 rounding (|z| <= 6, 300 rows: 300 * 6 * 2^-53 ~ 2e-13 absolute on a sum)."""
    N, D, K = sum(sizes), 6, 9
    z, idx, cs, w = _draw(N, D, K, 11, skew=True)
    st = [M.stats(z[lo:hi], idx[lo:hi], K) for lo, hi in M.cut(N, sizes)]
    got, ref = M.apply(st, cs, w, 0.95), R.ema_update(z, idx, cs, w, 0.95)
    assert torch.equal(got["N"], ref["N"])
    torch.testing.assert_close(got["m"], ref["m"], rtol=0, atol=1e-12)
    torch.testing.assert_close(got["e"], ref["e"], rtol=1e-12, atol=1e-12)
    assert torch.equal(torch.stack(st)[:, :, 0].sum(0), torch.bincount(idx, minlength=K).double())


def test_restart_takes_the_row_of_the_shard_the_two_uniforms_name():
    D, K = 3, 6
    sizes = (4, 1, 7)                                                                  # a shard of one row
    N = sum(sizes)
    z, idx, cs, w = _draw(N, D, K, 5)
    below1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    v = torch.tensor([0.0, below1, 0.34, 0.5, 0.99, 0.0])                              # the shard: floor(v * 3)
    u = torch.tensor([0.0, below1, 0.5, below1, 0.0, 0.26])                            # the row inside every shard: floor(u * N_s)
    bounds = M.cut(N, sizes)
    st = [M.stats(z[lo:hi], idx[lo:hi], K, u) for lo, hi in bounds]
    out = M.apply(st, torch.zeros(K), w, 0.5, 1e-5, 1e9, v)                            # every code is below the threshold
    assert out["dead"].all() and out["shard"].tolist() == [0, 2, 1, 1, 2, 0]
    want_rows = [0 + 0, 5 + 6, 4 + 0, 4 + 0, 5 + 0, 0 + 1]                             # shard's first row + floor(u * N_s)
    assert torch.equal(out["e"], z[want_rows].double())
    assert M.pick(torch.tensor([below1]), 1).item() == 0 and M.pick(torch.tensor([below1]), 1 << 24).item() == (1 << 24) - 1
    none = M.apply(st, torch.full((K,), 50.0), w, 0.5, 1e-5, 1.0, v)                   # nothing below the threshold: no restart
    assert not none["dead"].any() and torch.equal(none["e"], M.apply([s[:, :D + 1] for s in st], torch.full((K,), 50.0), w, 0.5)["e"])
    # N and m stay as updated
    assert torch.equal(out["m"], M.apply([s[:, :D + 1] for s in st], torch.zeros(K), w, 0.5)["m"])


# ---- the kernels' text on the host -------------------------------------------------------------------------------------------------

def _kernel_order_apply(st, cs, w, decay, eps, thr, v):
    """the apply in the kernels' own order, in numpy fp64 (one operation per line of vq_ema_merge.h): -> nk, n, cluster, m, e"""
    st = st.numpy()
    R_, K, C = st.shape
    D = w.shape[1]
    cnt = st[0, :, 0].copy()
    S = st[0, :, 1:D + 1].copy()
    for r in range(1, R_):
        cnt = cnt + st[r, :, 0]
        S = S + st[r, :, 1:D + 1]
    nk = decay * cs.numpy().astype(np.float64) + (1.0 - decay) * cnt
    per = (K + 1023) // 1024
    part = np.zeros(1024)
    for t in range(1024):
        local = 0.0
        for j in range(per):
            if t * per + j < K:
                local += nk[t * per + j]
        part[t] = local
    o = 512
    while o > 0:
        part[:o] = part[:o] + part[o:2 * o]
        o >>= 1
    n = part[0]
    m = decay * w.numpy().astype(np.float64) + (1.0 - decay) * S
    e = m / ((nk + eps) / (n + float(K) * eps) * n)[:, None]
    if thr is not None and thr >= 0:
        j = M.pick(v, R_).numpy()
        for k in range(K):
            if nk[k] < thr:
                e[k] = st[j[k], k, D + 1:]
    return nk, np.float64(n), nk.astype(np.float32), m.astype(np.float32), e.astype(np.float32)


def test_kernel_text_on_the_host(tmp_path):
    """tests/host/ema_merge_harness.cpp compiles csrc/vq_ema_merge.h -- the whole bodies of the pack, count and apply kernels -- for
    the host with AddressSanitizer and UBSan and -ffp-contract=off, runs them over the cases written here (ragged maps, a shard of one
    row, K past one code per thread of the count kernel, R = 1 / 3 / 8, restart with u = 0 and u just below 1, a NaN candidate) and
    compares every output bit for bit."""
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe, data = str(tmp_path / "ema_merge_harness"), str(tmp_path / "cases.bin")
    below1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    blobs = []
    # pack: (B, H, W, D, K, row_uniforms?)
    for B, H, W, D, K, has_u in ((3, 3, 3, 5, 7, 1), (3, 3, 3, 5, 7, 0), (1, 1, 1, 1, 1, 1), (2, 2, 5, 4, 300, 1), (1, 4, 4, 256, 16, 1)):
        N = B * H * W
        z, idx, _, _ = _draw(N, D, K, N + D)
        u = torch.rand(K, generator=torch.Generator().manual_seed(K))
        u[0], u[-1] = 0.0, below1
        want = M.stats(z, idx, K, u if has_u else None)
        offsets = np.concatenate([[0], np.cumsum(np.bincount(idx.numpy(), minlength=K))]).astype(np.int32)
        blobs.append(struct.pack("6i", N, K, D, H * W, has_u, 0) + z.numpy().tobytes() + offsets.tobytes() +
                     want[:, 1:D + 1].contiguous().numpy().tobytes() + (u.numpy().tobytes() if has_u else b"") + want.numpy().tobytes())
    # apply: (sizes of the shards, D, K, threshold)
    for sizes, D, K, thr in (((30,), 5, 7, None), ((30,), 5, 7, 4.0), ((9, 1, 20), 3, 6, 3.0), ((5,) * 8, 2, 2500, 0.004),
                             ((4, 4, 4), 256, 3, None), ((1,), 1, 1, 0.0), ((7, 8), 4, 5, -1.0)):
        N = sum(sizes)
        z, idx, cs, w = _draw(N, D, K, N + K, skew=True)
        has_u = thr is not None
        g = torch.Generator().manual_seed(N)
        u, v = torch.rand(K, generator=g), torch.rand(K, generator=g)
        v[0], v[-1] = 0.0, below1
        st = torch.stack([M.stats(z[lo:hi], idx[lo:hi], K, u if has_u else None) for lo, hi in M.cut(N, sizes)])
        if has_u and K > 2:
            st[len(sizes) - 1, K - 1, D + 1] = float("nan")                          # a NaN candidate: stays in code K - 1's row
        nk, n, c32, m32, e32 = _kernel_order_apply(st, cs, w, 0.9, 1e-5, thr, v)
        if has_u and thr >= 0:
            ref = M.apply(st, cs, w, 0.9, 1e-5, thr, v)                              # the kernel-order values against the restatement
            live = ~ref["dead"].numpy()
            np.testing.assert_allclose(e32[live], ref["e"].numpy()[live], rtol=3e-7)
            assert np.array_equal(e32[~live], ref["e"].numpy()[~live].astype(np.float32), equal_nan=True)
            assert not np.isnan(e32[live]).any()
        blobs.append(struct.pack("6i", N, K, D, 1, int(has_u), len(sizes)) + struct.pack("3d", 0.9, 1e-5, thr if has_u else -1.0) +
                     st.numpy().tobytes() + (v.numpy().tobytes() if has_u else b"") + cs.numpy().tobytes() + w.numpy().tobytes() +
                     nk.tobytes() + n.tobytes() + c32.tobytes() + m32.tobytes() + e32.tobytes())
    with open(data, "wb") as f:
        f.write(struct.pack("i", len(blobs)) + b"".join(blobs))
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "ema_merge_harness.cpp")])
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

NAMES = ("vqvae_vq_ema_stats_workspace_bytes", "vqvae_vq_ema_stats_f32", "vqvae_vq_ema_apply_workspace_bytes", "vqvae_vq_ema_apply_f32")


def test_entries_are_declared_and_bound_and_the_abi_stays_9():
    import ctypes
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    src = open(os.path.join(ROOT, "include", "vqvae_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"VQVAE_API\s+(int|size_t)\s+" + name + r"\s*\(", src)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 13, 3, 15]
    assert _lib.load().vqvae_abi_version() == 9 and re.search(r"#define VQVAE_HIP_ABI_VERSION 9\b", src)
    assert "vq_ema_merge.hip" in [os.path.basename(s) for s in build.sources()]


def test_the_sizing_calls_and_the_argument_errors_come_back_before_any_launch():
    from vqvae_amd import _lib
    L = _lib.load()
    ssize, asize = L.vqvae_vq_ema_stats_workspace_bytes, L.vqvae_vq_ema_apply_workspace_bytes
    assert ssize(2048, 512, 64) == L.vqvae_vq_backward_workspace_bytes(2048, 512, 64) and ssize(1, 1, 1) > 0
    for bad in ((0, 512, 64), (1 << 31, 512, 64), (2048, 0, 64), (2048, 16385, 64), (2048, 512, 0), (2048, 512, 257)):
        assert ssize(*bad) == 0, bad
    assert asize(1, 512, 64) >= 513 * 8 and asize(1024, 16384, 256) == asize(1, 16384, 256)
    for bad in ((0, 512, 64), (1025, 512, 64), (1, 0, 64), (1, 16385, 64), (1, 512, 0), (1, 512, 257), (-1, 512, 64)):
        assert asize(*bad) == 0, bad
    P = 1 << 24                                                # fake, aligned, disjoint "device pointers" (never dereferenced)
    z, idx, u, stats, ws, cs, w, cb = [P * (i + 1) for i in range(8)]

    def S(**k):
        a = dict(z=z, idx=idx, B=2, D=16, H=4, W=4, K=64, u=None, flags=0, stats=stats, ws=ws, n=1 << 30)
        a.update(k)
        return L.vqvae_vq_ema_stats_f32(a["z"], a["idx"], a["B"], a["D"], a["H"], a["W"], a["K"], a["u"], a["flags"], a["stats"], a["ws"],
                                        a["n"], None)

    def A(**k):
        a = dict(stats=stats, R=2, K=64, D=16, C=17, decay=0.99, eps=1e-5, thr=-1.0, v=None, cs=cs, w=w, cb=cb, ws=ws, n=1 << 30)
        a.update(k)
        return L.vqvae_vq_ema_apply_f32(a["stats"], a["R"], a["K"], a["D"], a["C"], a["decay"], a["eps"], a["thr"], a["v"], a["cs"],
                                        a["w"], a["cb"], a["ws"], a["n"], None)

    for name in ("z", "idx", "stats"):
        assert S(**{name: None}) == -1, name
    for name in ("stats", "cs", "w", "cb"):
        assert A(**{name: None}) == -1, name
    assert S(B=0) == -2 and S(D=0) == -2 and S(K=0) == -2 and S(H=0) == -2 and A(K=0) == -2 and A(D=0, C=1) == -2
    assert S(D=257) == -3 and S(K=16385) == -3 and S(flags=2) == -3 and S(flags=1 | 0x800) == -3 and S(B=1 << 29, H=2, W=2) == -3
    assert S(stats=stats + 4) == -3 and A(stats=stats + 4) == -3                       # not 8-byte aligned
    assert A(R=0) == -3 and A(R=1025) == -3 and A(R=-1) == -3 and A(D=257, C=258) == -3 and A(K=16385) == -3
    assert A(C=16) == -3 and A(C=32) == -3 and A(C=34) == -3                          # C is D + 1 or 2 D + 1
    assert A(v=u, thr=1.0) == -3                                                    # shard_uniforms with C = D + 1
    assert A(decay=1.5) == -3 and A(decay=-0.1) == -3 and A(decay=float("nan")) == -3 and A(eps=0.0) == -3
    assert S(ws=None) == -4 and S(n=16) == -4 and A(ws=None) == -4 and A(n=64 * 8) == -4


def test_front_ends_reject_cpu_tensors_and_bad_shapes():
    from vqvae_amd import _lib, functional as F
    z, idx = torch.zeros(1, 4, 2, 2), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_ema_stats(z, idx, 8)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_ema_apply(torch.zeros(1, 8, 5, dtype=torch.float64), torch.zeros(8), torch.zeros(8, 4), torch.zeros(8, 4), 0.9)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_ema_stats_workspace(0, 8, 4, "cpu")
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_ema_apply_workspace(1025, 8, 4, "cpu")
    assert F.vq_ema_stats.__kwdefaults__ == {"row_uniforms": None, "rowmajor": False, "workspace": None, "out": None}
    assert F.vq_ema_apply.__kwdefaults__ == {"threshold": None, "shard_uniforms": None, "workspace": None}


# ---- construction on the CPU ------------------------------------------------------------------------------------------------------

DIMS = (32, 8, 1, 64, 16, 0.25)


def test_the_default_is_todays_model():
    from vqvae_amd.modules import VQVAE, FactorizedVectorQuantizerEMA, GroupedVectorQuantizerEMA, VectorQuantizerEMA
    for kw, cls in ((dict(), VectorQuantizerEMA), (dict(codebook_dim=4), FactorizedVectorQuantizerEMA),
                    (dict(codebook_groups=2), GroupedVectorQuantizerEMA), (dict(restart_threshold=1.0, cosine_sim=True), VectorQuantizerEMA)):
        models, after = [], []
        for extra in (dict(), dict(ema_sync=False, ema_accumulate=1), dict(ema_sync=True, ema_accumulate=4)):
            torch.manual_seed(0)
            models.append(VQVAE(*DIMS, ema_decay=0.99, **kw, **extra))
            after.append(torch.rand(4))
        for m, a in zip(models[1:], after[1:]):
            assert type(m.vector_quantization) is cls and torch.equal(after[0], a)      # no random number drawn on the way
            assert list(models[0].state_dict()) == list(m.state_dict())
            for k, v in models[0].state_dict().items():
                assert torch.equal(v, m.state_dict()[k]), k
        vq = models[1].vector_quantization
        assert (vq.ema_sync, vq.ema_accumulate, vq.pending_ema_updates) == (False, 1, 0) and not vq._ema_merging
        vq = models[2].vector_quantization
        assert (vq.ema_sync, vq.ema_accumulate, vq.pending_ema_updates) == (True, 4, 0) and vq._ema_merging
        vq.flush_ema_()                                                                 # nothing pending: nothing happens, on any device


def test_the_constructor_rules():
    import inspect
    from vqvae_amd.modules import VQVAE, FactorizedVectorQuantizerEMA, GroupedVectorQuantizerEMA, VectorQuantizerEMA
    for kw in (dict(ema_sync=True), dict(ema_accumulate=2), dict(ema_sync=True, codebook_groups=2), dict(ema_accumulate=3, n_quantizers=2)):
        with pytest.raises(ValueError):
            VQVAE(*DIMS, **kw)
    for bad in (0, -1, 1025, 2.0, True, None, "2"):
        with pytest.raises(ValueError):
            VQVAE(*DIMS, ema_decay=0.99, ema_accumulate=bad)
        with pytest.raises(ValueError):
            VectorQuantizerEMA(64, 16, 0.25, accumulate=bad)
        with pytest.raises(ValueError):
            GroupedVectorQuantizerEMA(2, 64, 16, 0.25, accumulate=bad)
    assert VQVAE(*DIMS, ema_decay=0.99, ema_accumulate=1024).vector_quantization.ema_accumulate == 1024
    assert FactorizedVectorQuantizerEMA(64, 16, 4, 0.25, sync=True, accumulate=2).ema_sync
    names = list(inspect.signature(VQVAE.__init__).parameters)
    i = names.index("ema_sync")                                                         # in front of codebook_dim, which stays the last
    assert names[i + 1] == "ema_accumulate" and i > names.index("ema_decay") and names[-1] == "codebook_dim"
    p = inspect.signature(VQVAE.__init__).parameters
    assert p["ema_sync"].kind is p["ema_accumulate"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls, args in ((VectorQuantizerEMA, (64, 16, 0.25)), (FactorizedVectorQuantizerEMA, (64, 16, 4, 0.25)),
                      (GroupedVectorQuantizerEMA, (2, 64, 16, 0.25))):
        p = inspect.signature(cls.__init__).parameters
        assert p["sync"].kind is p["accumulate"].kind is inspect.Parameter.KEYWORD_ONLY
        assert (p["sync"].default, p["accumulate"].default) == (False, 1)
    # the collectives are reached through two attributes an instance may replace
    from vqvae_amd import sharding
    vq = VectorQuantizerEMA(64, 16, 0.25, sync=True)
    t = torch.zeros(2, 3, 4, dtype=torch.float64)
    assert vq._ema_gather(t) is t and vq._ema_broadcast(t) is t and sharding.all_gather_ema_stats(t) is t   # no group: no collective


def test_models_with_the_options_pickle_and_deepcopy():
    import copy
    import io
    from vqvae_amd.modules import VQVAE
    m = VQVAE(*DIMS, ema_decay=0.99, ema_sync=True, ema_accumulate=2)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    for c in (torch.load(buf, weights_only=False), copy.deepcopy(m)):
        vq = c.vector_quantization
        assert (vq.ema_sync, vq.ema_accumulate, vq.pending_ema_updates) == (True, 2, 0)
        c.load_state_dict(m.state_dict())


def test_train_tool_options_are_absent_unless_given():
    src = open(os.path.join(ROOT, "tools", "train_checkpoint.py")).read()
    for opt in ("--ema_accumulate", "--ema_sync"):
        line = next(l for l in src.splitlines() if f'"{opt}"' in l)
        assert "argparse.SUPPRESS" in line
    from tools import train_checkpoint as tc
    assert tc.parse([])[1] == {}
    assert tc.parse(["--ema_decay", "0.99", "--ema_accumulate", "2", "--ema_sync"])[1] == dict(ema_decay=0.99, ema_accumulate=2, ema_sync=True)


# ---- the collectives on a 2-rank gloo group ------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_inputs(rank):
    """rank `rank`'s two micro-batches: (z, idx) with sizes that differ between the ranks"""
    out = []
    for a in range(2):
        N = 20 + 7 * rank + 3 * a
        z, idx, _, _ = _draw(N, 4, 6, 100 + 10 * rank + a)
        out.append((z, idx))
    return out


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vqvae_amd import sharding
    u = torch.rand(2, 6, generator=torch.Generator().manual_seed(50 + rank))           # every rank draws its own
    sharding.broadcast_ema_uniforms(u)
    mine = torch.stack([M.stats(z, idx, 6, u[1]) for z, idx in _rank_inputs(rank)])
    before = mine.clone()
    got = sharding.all_gather_ema_stats(mine)
    q.put((rank, u.numpy().tobytes(), got.numpy().tobytes(), tuple(got.shape), bool(torch.equal(mine, before))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gather_is_rank_major_and_the_uniforms_are_rank_zeros():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    u0 = torch.rand(2, 6, generator=torch.Generator().manual_seed(50))
    assert res[0][1] == res[1][1] == u0.numpy().tobytes()                               # rank 0's uniforms everywhere
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3] == (4, 6, 9)               # the same bytes on both ranks
    assert res[0][4] and res[1][4]                                                      # the input is left as it was
    got = torch.from_numpy(np.frombuffer(res[0][2], dtype=np.float64).copy()).reshape(4, 6, 9)
    shards = [s for r in range(world) for s in _rank_inputs(r)]                         # rank-major, each rank's in order
    want = torch.stack([M.stats(z, idx, 6, u0[1]) for z, idx in shards])
    assert torch.equal(got, want)
    # the restatement's apply on what arrived is the apply on the concatenated shards
    _, _, cs, w = _draw(1, 4, 6, 9)
    a, b = M.apply(got, cs, w, 0.9, 1e-5, 3.0, u0[0]), M.apply(want, cs, w, 0.9, 1e-5, 3.0, u0[0])
    for k in ("N", "m", "e"):
        assert torch.equal(a[k], b[k]), k
    whole = R.ema_update(torch.cat([z for z, _ in shards]), torch.cat([i for _, i in shards]), cs, w, 0.9)
    assert torch.equal(a["N"], whole["N"])
    torch.testing.assert_close(a["m"], whole["m"], rtol=0, atol=1e-12)
