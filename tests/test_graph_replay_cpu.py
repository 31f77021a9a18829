"""The input states of tests/test_graph_replay_gpu.py do what they are there for (no GPU needed).

A replay that leaves the histogram, a flag word or a per-image maximum of the replay before it in place only shows when
consecutive replays make those words differ.  Checked here, on the host, in fp64:
  part 1  the rows of state b and of state c select non-empty, disjoint index sets of at most K/4 codes each;
  part 2  the per-image scale rotation moves every image's maximum by at least 2^6 in each direction over the schedule."""
import numpy as np
import pytest

from tests import graph_replay as G


@pytest.mark.parametrize("case", sorted(G.VQ_CASES))
def test_vq_states_select_disjoint_bounded_code_sets(case):
    c = G.VQ_CASES[case]
    K, D = c["K"], c["D"]
    n = G.B_VQ * c["H"] * c["W"]
    assert n <= 192
    cb = G.vq_codebook(case)
    a, b, cc, a2 = G.vq_states(case)
    assert a2 is a and all(s.shape == (n, D) and s.dtype == np.float32 for s in (a, b, cc))
    ib, ic = set(G.argmin_fp64(b, cb).tolist()), set(G.argmin_fp64(cc, cb).tolist())
    limit = 2 if K == 5 else K // 4
    assert ib and ic, "an empty index set"
    assert not (ib & ic), f"states b and c share codes {sorted(ib & ic)}"
    assert len(ib) <= limit and len(ic) <= limit
    (b0, b1), (c0, c1) = G.vq_code_ranges(K)
    assert all(b0 <= k < b1 for k in ib) and all(c0 <= k < c1 for k in ic)
    assert b1 <= c0
    # the noise is 2^-10 of the code's norm
    jb = G.argmin_fp64(b, cb)
    rel = np.linalg.norm(b.astype(np.float64) - cb[jb], axis=1) / np.linalg.norm(cb[jb].astype(np.float64), axis=1)
    assert np.all(rel < 2.0 ** -9) and np.all(rel > 2.0 ** -11)
    # state a is not confined to either set: a full replay between and after the two partial ones
    ia = set(G.argmin_fp64(a, cb).tolist())
    assert ia - ib and ia - ic
    # the layout is a permutation of the rows
    z = G.vq_layout(case, b)
    assert z.shape == ((G.B_VQ, c["H"], c["W"], D) if c["rowmajor"] else (G.B_VQ, D, c["H"], c["W"]))
    back = z if c["rowmajor"] else z.transpose(0, 2, 3, 1)
    assert np.array_equal(back.reshape(n, D), b)


def test_vq_cases_cover_the_sizes_the_issue_names():
    assert G.VQ_CASES["track_k1000"]["K"] * 4 == 4000                                   # the 4000-byte histogram clear
    f = G.VQ_CASES["filter_nchw_7x7"]
    assert (f["H"] * f["W"]) % 32 != 0 and not f["rowmajor"]
    assert len(G.VQ_CASES) == 9


@pytest.mark.parametrize("case", sorted(G.MODEL_CASES))
def test_image_scale_rotation_moves_every_maximum_both_ways(case):
    c = G.MODEL_CASES[case]
    xs = G.model_images(case)
    assert len(xs) == G.N_REPLAYS == 5 and np.array_equal(xs[0], xs[4])
    assert G.SCALES == (1.0, 2.0 ** -9, 2.0 ** 6, 0.0)
    for i in range(c["B"]):
        m = [float(np.abs(x[i]).max()) for x in xs]
        assert min(m) == 0.0, f"image {i} is never all-zero"
        steps = list(zip(m[:-1], m[1:]))
        # between two NON-ZERO maxima (so the all-zero image does not stand in for either direction) ...
        up = [q / p for p, q in steps if p > 0 and q > 0 and q > p]
        down = [p / q for p, q in steps if p > 0 and q > 0 and q < p]
        assert up and max(up) >= 2.0 ** 6, f"image {i}: maxima {m} never rise by 2^6"
        assert down and max(down) >= 2.0 ** 6, f"image {i}: maxima {m} never fall by 2^6"
        # ... and through the all-zero image in both directions as well
        assert any(p > 0 and q == 0 for p, q in steps) and any(p == 0 and q > 0 for p, q in steps)
        assert [G.image_scale(i, r) for r in range(5)] == [G.SCALES[(i + r) % 4] for r in range(4)] + [G.SCALES[i % 4]]


@pytest.mark.parametrize("case", sorted(G.MODEL_CASES))
def test_decode_index_states_use_disjoint_code_subsets(case):
    c = G.MODEL_CASES[case]
    K = c["dims"][3]
    idx = G.model_indices(case)
    assert len(idx) == G.N_REPLAYS and np.array_equal(idx[0], idx[4])
    n = c["B"] * (c["HW"] // 4) ** 2
    for r in range(G.N_REPLAYS - 1):
        assert idx[r].shape == (n, 1) and idx[r].dtype == np.int64 and idx[r].min() >= 0 and idx[r].max() < K
        assert not (set(idx[r].ravel().tolist()) & set(idx[r + 1].ravel().tolist())) or r == 3
    assert not (set(idx[3].ravel().tolist()) & set(idx[4].ravel().tolist()))


def test_step_cases_are_the_issues():
    s = G.STEP_CASES
    assert sum(1 for c in s.values() if c.get("max_grad_norm")) == 1
    assert s["fsq"]["dims"][3] == 8 * 5 * 5 * 5 and s["rvq2"]["dims"][3] == 64
    assert (s["default_b8"]["dims"], s["default_b8"]["B"]) == ((128, 32, 2, 512, 64), 8)
    assert (s["generic_16x16"]["dims"], s["generic_16x16"]["B"], s["generic_16x16"]["HW"]) == ((64, 16, 1, 64, 32), 6, 16)
    assert all("restart_threshold" not in c["kw"] for c in s.values())
    xs = G.step_images("plain", 3)
    assert not np.array_equal(xs[0], xs[1]) and not np.array_equal(xs[1], xs[2])
