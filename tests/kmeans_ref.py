"""fp64 restatement, on the CPU, of the k-means initialisation of the codebook (include/vqvae_hip.h: vqvae_vq_kmeans_seed_f32,
vqvae_vq_kmeans_update_f32; the operation order is the header of vqvae_amd/csrc/vq_kmeans.hip, mirrored here step for step).
numpy float64 and Python floats are IEEE fp64 with one rounding per operation, which is what the kernels compute.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

BLOCK = 256          # rows per selection block
GROUPS = 256         # groups of consecutive blocks


def _rows64(z):
    """(N, D) rows (numpy or torch, fp32) -> the same values in float64 (exact)"""
    z = z.detach().cpu().numpy() if hasattr(z, "detach") else np.asarray(z)
    assert z.dtype == np.float32 and z.ndim == 2
    return z.astype(np.float64)


def uniform_row(u, N):
    """min(floor(double(u) N), N - 1) for an fp32 uniform"""
    return int(min(max(np.floor(np.float64(np.float32(u)) * np.float64(N)), 0.0), N - 1))


def _descend(sums, first, thr, base):
    """one level of the pick: items `sums` (numbered from `first`) scanned in order from the running prefix `base`
    -> (selected item or -1, its base)"""
    run, last, last_base = base, -1, base
    for i, s in enumerate(sums):
        inc = run + s
        if s > 0.0:
            last, last_base = first + i, run
            if inc > thr:
                return first + i, run
        run = inc
    return last, last_base


def _pick(w, S, u, N):
    """the row a round picks from the weights w (N,) and their block sums S (nb,), all Python / numpy fp64"""
    nb = len(S)
    per = -(-nb // GROUPS)
    G = []
    for t in range(GROUPS):
        g = 0.0
        for b in range(t * per, min((t + 1) * per, nb)):
            g = g + float(S[b])
        G.append(g)
    T = 0.0
    for g in G:
        T = T + g
    if not T > 0.0:
        return uniform_row(u, N), T
    thr = float(np.float64(np.float32(u))) * T
    t, base = _descend(G, 0, thr, 0.0)
    b0 = t * per
    b, base = _descend([float(s) for s in S[b0:min(b0 + per, nb)]], b0, thr, base)
    r, _ = _descend([float(v) for v in w[b * BLOCK:min((b + 1) * BLOCK, N)]], b * BLOCK, thr, base)
    return r, T


def _block_sums(w):
    """S_b: block_sum_f64's tree (red[i] += red[i + o], o = 128 ... 1) over each block of 256 weights, zeros past N"""
    N = w.shape[0]
    nb = -(-N // BLOCK)
    red = np.zeros(nb * BLOCK, dtype=np.float64)
    red[:N] = w
    red = red.reshape(nb, BLOCK).copy()
    o = BLOCK // 2
    while o > 0:
        red[:, :o] = red[:, :o] + red[:, o:2 * o]
        o >>= 1
    return red[:, 0].copy()


def seed(z, K, uniforms, trace=None):
    """k-means++ seeding of K codes on the rows z (N, D) fp32 from K fp32 uniforms -> rows (K,) int64.
    Vectorised over the rows; the channel loop stays a loop (its order is the contract).  trace: a list that receives, per round
    k >= 1, (w before the pick, T)."""
    z64 = _rows64(z)
    N, D = z64.shape
    u = np.asarray(uniforms.detach().cpu().numpy() if hasattr(uniforms, "detach") else uniforms, dtype=np.float32)
    rows = np.empty(K, dtype=np.int64)
    rows[0] = uniform_row(u[0], N)
    w = None
    for k in range(1, K):
        e = z64[rows[k - 1]]
        dist = np.zeros(N, dtype=np.float64)
        for c in range(D):
            d = z64[:, c] - e[c]
            dist = dist + d * d
        w = dist if k == 1 else np.where(dist < w, dist, w)
        rows[k], T = _pick(w, _block_sums(w), u[k], N)
        if trace is not None:
            trace.append((w.copy(), T))
    return rows


def seed_loop(z, K, uniforms):
    """the same seeding written as plain loops over rows, channels, blocks and groups (checks the vectorised restatement)"""
    z64 = _rows64(z)
    N, D = z64.shape
    zl = z64.tolist()
    u = [float(np.float32(v)) for v in (uniforms.tolist() if hasattr(uniforms, "tolist") else uniforms)]
    rows = [min(int(u[0] * N // 1), N - 1)]
    w = [0.0] * N
    nb = -(-N // BLOCK)
    per = -(-nb // GROUPS)
    for k in range(1, K):
        e = zl[rows[k - 1]]
        for n in range(N):
            acc = 0.0
            for c in range(D):
                d = zl[n][c] - e[c]
                acc = acc + d * d
            w[n] = acc if k == 1 or acc < w[n] else w[n]
        S = []
        for b in range(nb):
            red = [w[b * BLOCK + i] if b * BLOCK + i < N else 0.0 for i in range(BLOCK)]
            o = BLOCK // 2
            while o > 0:
                for i in range(o):
                    red[i] = red[i] + red[i + o]
                o >>= 1
            S.append(red[0])
        G = []
        for t in range(GROUPS):
            g = 0.0
            for b in range(t * per, min((t + 1) * per, nb)):
                g = g + S[b]
            G.append(g)
        T = 0.0
        for g in G:
            T = T + g
        if not T > 0.0:
            rows.append(min(int(u[k] * N // 1), N - 1))
            continue
        thr = u[k] * T

        def scan(items, first, base):
            run, sel, sel_base, last, last_base = base, -1, base, -1, base
            for i in range(len(items)):
                s = items[i]
                inc = run + s
                if s > 0.0:
                    last, last_base = first + i, run
                    if inc > thr:
                        sel, sel_base = first + i, run
                        break
                run = inc
            return (sel, sel_base) if sel >= 0 else (last, last_base)

        t, base = scan(G, 0, 0.0)
        b, base = scan(S[t * per:min((t + 1) * per, nb)], t * per, base)
        r, _ = scan(w[b * BLOCK:min((b + 1) * BLOCK, N)], b * BLOCK, base)
        rows.append(r)
    return np.asarray(rows, dtype=np.int64)


def update(z, idx, codebook, uniforms=None):
    """one Lloyd mean update: z (N, D) fp32 rows, idx (N,) codes, codebook (K, D) fp32 -> (new codebook in float64 -- means
    unrounded, kept / restarted codes the fp32 values exactly --, counts (K,) int64)"""
    z64 = _rows64(z)
    cb = _rows64(codebook).copy()
    idx = np.asarray(idx.detach().cpu().numpy() if hasattr(idx, "detach") else idx).reshape(-1).astype(np.int64)
    K, N = cb.shape[0], z64.shape[0]
    counts = np.bincount(idx, minlength=K).astype(np.int64)
    s = np.zeros_like(cb)
    np.add.at(s, idx, z64)
    have = counts > 0
    cb[have] = s[have] / counts[have, None].astype(np.float64)
    if uniforms is not None:
        u = np.asarray(uniforms.detach().cpu().numpy() if hasattr(uniforms, "detach") else uniforms, dtype=np.float32)
        for k in np.nonzero(~have)[0]:
            cb[k] = z64[uniform_row(u[k], N)]
    return cb, counts


def update_loop(z, idx, codebook, uniforms=None):
    """the same update as a per-row loop"""
    z64 = _rows64(z).tolist()
    cb = _rows64(codebook).tolist()
    idx = [int(v) for v in np.asarray(idx.detach().cpu().numpy() if hasattr(idx, "detach") else idx).reshape(-1)]
    K, D, N = len(cb), len(cb[0]), len(z64)
    c = [0] * K
    s = [[0.0] * D for _ in range(K)]
    for n in range(N):
        c[idx[n]] += 1
        for d in range(D):
            s[idx[n]][d] += z64[n][d]
    for k in range(K):
        if c[k] > 0:
            cb[k] = [s[k][d] / float(c[k]) for d in range(D)]
        elif uniforms is not None:
            cb[k] = list(z64[min(int(float(np.float32(uniforms[k])) * N // 1), N - 1)])
    return np.asarray(cb, dtype=np.float64), np.asarray(c, dtype=np.int64)


def assign(z, codebook):
    """the quantizer's indices (first-index ties, the reference's fp32 arithmetic) of the rows z (N, D) against codebook (K, D):
    the C oracle's restatement of models/quantizer.py:49-54"""
    from oracle import c_oracle
    z = z.detach().cpu().numpy() if hasattr(z, "detach") else np.asarray(z)
    cb = codebook.detach().cpu().numpy() if hasattr(codebook, "detach") else np.asarray(codebook)
    return np.asarray(c_oracle.vq_indices_rows(z.astype(np.float32), cb.astype(np.float32), threads=1)).reshape(-1).astype(np.int64)


def kmeans(z, K, iters, seed_uniforms, round_uniforms=None):
    """whole k-means: seeding from seed_uniforms (K,), then `iters` rounds of assign + update (round_uniforms: None, or (iters, K)
    uniforms that reseed empty codes); the codebook is rounded to fp32 after every update, as the kernel stores it
    -> (codebook (K, D) fp32, counts (K,) int64 of the last assignment, rows (K,) of the seeding)"""
    zf = z.detach().cpu().numpy() if hasattr(z, "detach") else np.asarray(z)
    rows = seed(zf, K, seed_uniforms)
    cb = zf[rows].copy()
    counts = np.zeros(K, dtype=np.int64)
    for t in range(iters):
        idx = assign(zf, cb)
        cb64, counts = update(zf, idx, cb, None if round_uniforms is None else round_uniforms[t])
        cb = cb64.astype(np.float32)
    return cb, counts, rows


def mean_sq_dist(z, codebook, idx):
    """mean over the rows of |z_n - e_idx_n|^2 in fp64"""
    z64, cb = _rows64(z), _rows64(codebook)
    idx = np.asarray(idx.detach().cpu().numpy() if hasattr(idx, "detach") else idx).reshape(-1)
    return float(((z64 - cb[idx]) ** 2).sum(1).mean())


# ---- data with known answers (shared by the CPU and GPU tests) ---------------------------------------------------------------------

def repeated_points(M, r, D, seed):
    """M distinct random points, each r times, shuffled -> (rows (M r, D) fp32, which point each row is (M r,))"""
    g = np.random.default_rng(seed)
    pts = g.standard_normal((M, D)).astype(np.float32)
    which = g.permutation(np.repeat(np.arange(M), r))
    return pts[which].copy(), which


def blobs(K, n, D, seed, spread=0.01, sep=1000.0):
    """K blobs of n rows each: centres on distinct corners of a cube of side sep * spread (any two at least sep spreads apart),
    every row within `spread` of its centre; shuffled -> (rows (K n, D) fp32, blob of each row (K n,), the least centre distance
    in spreads)"""
    assert K <= 2 ** min(D, 16)
    g = np.random.default_rng(seed)
    corners = np.array([[(b >> i) & 1 for i in range(D)] for b in range(K)], dtype=np.float64) * sep * spread
    noise = g.uniform(-1.0, 1.0, (K * n, D)) * spread / np.sqrt(D)            # |noise| <= spread
    which = g.permutation(np.repeat(np.arange(K), n))
    rows = (corners[which] + noise).astype(np.float32)
    d = np.sqrt(((corners[:, None, :] - corners[None, :, :]) ** 2).sum(-1))
    return rows, which, float(d[~np.eye(K, dtype=bool)].min() / spread) if K > 1 else float("inf")
