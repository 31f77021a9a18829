"""tests/grid_caps.py against the sources and against the tests it names: every kernel under vqvae_amd/csrc that uses gridDim.x has
a row; every row's kernel and anchors are still in the source; every covering test exists and its shape gives more units than
cap * 256, with a last lap that is neither empty nor whole and (where the unit count is not padded) ends inside a workgroup; for
the kernels with a scalar tail behind 4-wide laps the element count is no multiple of 4.  No GPU: the sources are read as text, the
shapes are imported."""
import glob
import importlib
import os
import re

import pytest

from tests import grid_caps as G

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vqvae_amd", "csrc")
FUNCTION = re.compile(r"\b(?:void|int|bool|float|double|auto)\s+(\w+)\s*\(([^;{}]*?)\)\s*\{", re.S)
ROWS = G.rows()
NUMERIC = [r for r in ROWS if isinstance(r.cap, int)]


def _source(name, root=CSRC):
    with open(os.path.join(root, name)) as f:
        return f.read()


def _code(text):
    """the text with // comments blanked (a comment that mentions gridDim.x is not a use)"""
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group()), text)


def grid_users(root=CSRC):
    """{(file, function)}: every function definition under `root` whose body mentions gridDim.x"""
    found = set()
    for path in sorted(glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.h"))):
        text = _code(_source(os.path.basename(path), root))
        defs = [(m.start(), m.group(1)) for m in FUNCTION.finditer(text)]
        for m in re.finditer(r"gridDim\.x", text):
            before = [n for p, n in defs if p < m.start()]
            assert before, f"{path}: gridDim.x outside any function"
            found.add((os.path.basename(path), before[-1]))
    return found


def missing_rows(root=CSRC, rows=ROWS):
    have = {(r.file, r.kernel) for r in rows}
    return sorted(f"{k} ({f})" for f, k in grid_users(root) - have)


def dead_rows(root=CSRC, rows=ROWS):
    """rows whose kernel no longer uses gridDim.x, or whose anchor text is gone from its file"""
    users, dead = grid_users(root), []
    for r in rows:
        if (r.file, r.kernel) not in users:
            dead.append(f"{r.kernel}: no function of that name uses gridDim.x in {r.file}")
        for f, text in r.anchors:
            if text not in _source(f, root):
                dead.append(f"{r.kernel}: {f} no longer holds `{text}`")
    return dead


def test_every_kernel_that_uses_the_grid_size_has_a_row():
    assert not missing_rows(), f"kernels without a row in tests/grid_caps.py: {missing_rows()}"
    names = [(r.file, r.kernel) for r in ROWS]
    assert len(names) == len(set(names))


def test_every_row_is_live():
    assert not dead_rows(), dead_rows()


def test_the_two_scans_notice_a_deleted_row_and_a_retuned_cap(tmp_path):
    """the checks above on a table without one row and on a copy of the sources with one cap literal changed: each names the kernel"""
    assert missing_rows(rows=[r for r in ROWS if r.kernel != "res_combine_kernel"]) == ["res_combine_kernel (conv_res.hip)"]
    for path in glob.glob(os.path.join(CSRC, "*.h*")):
        text = _source(os.path.basename(path))
        if path.endswith("vq_orthogonal.hip"):
            assert "grid_of((long long)K * D, 2048)" in text
            text = text.replace("grid_of((long long)K * D, 2048)", "grid_of((long long)K * D, 1024)")
        (tmp_path / os.path.basename(path)).write_text(text)
    dead = dead_rows(root=str(tmp_path))
    assert len(dead) == 1 and dead[0].startswith("orth_backward_kernel:"), dead


def _function_of(node):
    path, _, name = node.partition("::")
    assert path.startswith("tests/") and path.endswith(".py"), node
    mod = importlib.import_module(path[:-3].replace("/", "."))
    fn, _, case = name.partition("[")
    assert hasattr(mod, fn), f"{node}: no such test"
    return getattr(mod, fn), case.rstrip("]")


def _ids(fn):
    """the parametrize ids of a test with ONE parametrize mark (explicit ids, or the values joined the way pytest joins them)"""
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    if len(marks) != 1:
        return None
    values, ids = marks[0].args[1], marks[0].kwargs.get("ids")
    if isinstance(ids, (list, tuple)):
        return [str(i) for i in ids]
    if ids is not None:
        return None
    return ["-".join(str(x) for x in v) if isinstance(v, (list, tuple)) else str(v) for v in values]


@pytest.mark.parametrize("r", ROWS, ids=lambda r: r.kernel)
def test_covering_tests_exist(r):
    """every row names a test past its cap, or carries the arithmetic that shows there is no such shape"""
    if r.cap in (G.UNREACHABLE, G.NO_LOOP):
        assert not r.covers and r.note
        if r.cap == G.UNREACHABLE:
            assert r.proof() is True, f"{r.kernel}: the envelope now lets the loop lap"
        return
    assert r.covers, f"{r.kernel}: no covering test"
    for c in r.covers:
        fn, case = _function_of(c.node)
        ids = _ids(fn)
        if case and ids is not None:
            assert case in ids, f"{c.node}: the test has no such case ({ids})"
        assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", []) + [getattr(importlib.import_module(fn.__module__), "pytestmark", None)]
                   if m is not None), f"{c.node} is not a GPU test"


@pytest.mark.parametrize("r", NUMERIC, ids=lambda r: r.kernel)
def test_shapes_exceed_the_cap_with_a_ragged_last_lap(r):
    lap = r.cap * G.WG
    for c in r.covers:
        assert c.units > lap, f"{c.node}: {c.units} units do not exceed {r.kernel}'s {r.cap} workgroups of 256"
        last = c.units % lap
        assert 0 < last < lap, f"{c.node}: the last lap of {r.kernel} is empty or whole ({c.units} units, {lap} per lap)"
        if r.aligned:
            assert c.units % G.WG == 0, f"{r.kernel} is marked aligned, but {c.units} units are no multiple of 256"
        else:
            assert c.units % G.WG != 0, f"{c.node}: {r.kernel}'s last lap ends on a workgroup boundary ({c.units} units)"
        if c.elements is not None:
            assert c.elements % 4 != 0 and c.elements // 4 == c.units, f"{c.node}: no scalar tail behind the 4-wide laps"


@pytest.mark.parametrize("r", [r for r in ROWS if r.cap == G.CUS], ids=lambda r: r.kernel)
def test_persistent_grids_are_lapped_at_256_cus(r):
    """blocks the covering test's shape yields against the workgroups of the grid, from the host code's formula at 256 CUs"""
    for c in r.covers:
        if c.units is None:
            assert "depend on the data" in r.unit and r.note, f"{r.kernel}: no block count and no reason"
            continue
        assert c.units > c.elements, f"{c.node}: {c.units} blocks on {c.elements} workgroups do not lap {r.kernel}"


def test_image_maximum_cases_take_more_than_sixteen_laps():
    """act_absmax_kernel's row is about images past 64 parts: below that every thread already takes 16 laps (one part per 16384
    elements), so the cover must exceed 16 laps of 64 workgroups, the 1 048 576 elements the row names"""
    r = [r for r in ROWS if r.kernel == "act_absmax_kernel"][0]
    assert r.cap == 64 and r.covers
    for c in r.covers:
        assert 4 * c.units > 4 * 16 * r.cap * G.WG == 1048576, c.node


def test_persistent_rows_name_the_kernel_their_cover_launches():
    """the quantizer's own routing (the function the launch uses, asked through the library) for the covering shapes"""
    from tests import test_vq_gpu, test_vq_grouped_gpu
    from vqvae_amd import _lib, functional as F
    K, D, G_ = test_vq_grouped_gpu.CAP_SHAPE[:3]
    assert _lib.vq_kernel_name(512, 64, F.VQ_ROWMAJOR) == "vq_track_kernel_d64"
    B, H, W = test_vq_gpu.HEADLINE_SHAPES[1]
    assert _lib.vq_launch_form(B * H * W, 512, 64, H * W, F.VQ_ROWMAJOR)[:2] in G.TRACK_FORMS      # (the form this machine would launch)
    assert _lib.vq_kernel_name(512, 64, F.VQ_ROWMAJOR | F.VQ_BF16_FILTER) == "vq_filter_kernel_d64"
    assert _lib.vq_kernel_name(test_vq_gpu.GROUPS_CASE[0], test_vq_gpu.GROUPS_CASE[1], F.VQ_ROWMAJOR | F.VQ_EXACT_SWEEP) == "vq_exact_kernel"
    assert _lib.vq_kernel_name(K, D // G_, F.VQ_ROWMAJOR) == "vq_stream_sweep_kernel"
    assert _lib.vq_kernel_name(G.VQ_ANYD[0], G.VQ_ANYD[1], F.VQ_ROWMAJOR) == "vq_anyd_kernel"
    assert _lib.vq_kernel_name(G.VQ_ANYD[0], G.VQ_ANYD[1], F.VQ_ROWMAJOR | F.VQ_BF16_FILTER) == "vq_generic_kernel"


def test_pack_shapes_are_inside_their_entries_envelopes():
    """the weight-image cases are shapes the pack entries accept (a size query of 0 means refused)"""
    from vqvae_amd import _lib
    L = _lib.load()
    assert L.vqvae_conv_in_packed_bytes(*G.CONV_IN_PACK[:2]) > 0 and L.vqvae_convt_out_packed_bytes(*G.CONVT_OUT_PACK[:2]) > 0
    assert L.vqvae_conv_packed_bytes(1, *G.CONV_PACK[1:3]) > 0                      # VQVAE_CONV_3x3_S1
    assert L.vqvae_conv_in_packed_bytes(G.CONV_IN_MAX_CIN, G.CONV_IN_MAX_COUT) > 0
    assert L.vqvae_conv_in_packed_bytes(G.CONV_IN_MAX_CIN, G.CONV_IN_MAX_COUT + 1) == 0 and L.vqvae_conv_in_packed_bytes(5, 64) == 0
    K, dim, nl, ncls = G.SAMPLE_PACK[:4]
    assert L.vqvae_pixelcnn_sample_packed_bytes(K, dim, nl, ncls) > 0
    B, H, W, Cin, Cout, taps = G.TAPS_WGRAD
    assert L.vqvae_conv_taps_wgrad_workspace_bytes(28, Cin, Cout) > 0
    assert L.vqvae_conv_taps_pack_dgrad_bytes(G.taps_slice(28), G.TAPS_DGRAD[2], G.TAPS_DGRAD[3]) > 0
