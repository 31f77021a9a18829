"""CPU side of the GatedPixelCNN training path: the torch-autograd restatement the GPU tests use for shapes beyond the goldens is
pinned to the reference's recorded gradients, and the new C entries validate their arguments before launching anything."""
import os

import numpy as np
import pytest
import torch

from tests import pixelcnn_train_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pixelcnn_train_cases.npz"))


def _mirror_state(name):
    from vqvae_amd.pixelcnn import GatedPixelCNN
    K, dim, nl, ncls, B, H, W = R.CASES[name]
    torch.manual_seed(0)
    m = GatedPixelCNN(K, dim, nl, ncls)
    R.perturb_biases(m)
    return {k: v.detach().clone() for k, v in m.named_parameters()}


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_reference_gradients(name, golden):
    """fp64 restatement against the reference's fp32 autograd: loss, logits gradient and every recorded parameter gradient within
    the house tolerance (atol 1e-5 max|g| + rtol 1e-4)."""
    torch.set_num_threads(4)
    nl = R.CASES[name][2]
    x, label = R.inputs(name)
    loss, gl, grads = R.loss_and_grads(_mirror_state(name), x, label, nl)
    assert abs(float(loss) - float(golden[f"{name}/loss"])) <= 1e-5 * abs(float(golden[f"{name}/loss"]))
    got, ref, amax = R.at_stored(golden, f"{name}/grad_logits", gl.numpy())
    assert np.all(np.abs(got - ref) <= R.tolerance(ref, amax))
    keys = R.stored_names(golden, f"{name}/grad/")
    assert set(keys) == set(R.grad_keys(name, grads))
    for k in keys:
        got, ref, amax = R.at_stored(golden, f"{name}/grad/{k}", grads[k].numpy())
        assert np.all(np.abs(got - ref) <= R.tolerance(ref, amax)), k
        assert abs(float(grads[k].abs().max()) - amax) <= 1e-4 * amax + 1e-12, k        # the whole tensor's maximum too


def test_golden_covers_the_cases_the_issue_names(golden):
    """mask-'A' taps carry nonzero gradients, absent codes have zero embedding rows, the trajectory has three steps"""
    name = "k512_dim64_l15"
    for k, vertical in (("layers.0.vert_stack.weight", True), ("layers.0.horiz_stack.weight", False)):
        idx, val, _ = R.stored(golden, f"{name}/grad/{k}")
        shape = (128, 64, 4, 7) if vertical else (128, 64, 1, 4)
        masked = np.isin(idx, R.mask_a_positions(shape, vertical))
        assert masked.sum() >= 256 and np.abs(val[masked]).max() > 0, k
    x, _ = R.inputs(name)
    absent = np.setdiff1d(np.arange(512), x.numpy().ravel())
    idx, val, _ = R.stored(golden, f"{name}/grad/embedding.weight")
    rows = idx // 64
    assert np.isin(rows, absent).sum() >= 4 * 64 and np.all(val[np.isin(rows, absent)] == 0)
    assert len(golden["k64_dim32_l3/traj_loss"]) == 3


def test_new_entries_reject_bad_arguments_without_gpu():
    from vqvae_amd import _lib
    L = _lib.load()
    a = 256
    dy = (__import__("ctypes").c_int8 * 6)(-1, -1, -1, 0, 0, 0)
    dx = (__import__("ctypes").c_int8 * 6)(-1, 0, 1, -1, 0, 1)
    assert L.vqvae_conv_taps_wgrad_workspace_bytes(6, 64, 128) > 0
    assert L.vqvae_conv_taps_wgrad_workspace_bytes(33, 64, 128) == 0
    assert L.vqvae_conv_taps_wgrad_workspace_bytes(0, 64, 128) == 0
    assert L.vqvae_conv_taps_wgrad_workspace_bytes(6, 62, 128) == 0
    ws = L.vqvae_conv_taps_wgrad_workspace_bytes(6, 64, 128)
    assert L.vqvae_conv_taps_wgrad_f32(a, None, 1, 8, 8, 64, 128, 6, dy, dx, a, a, ws, None) == -1
    assert L.vqvae_conv_taps_wgrad_f32(a, a, 0, 8, 8, 64, 128, 6, dy, dx, a, a, ws, None) == -2
    assert L.vqvae_conv_taps_wgrad_f32(a, a, 1, 8, 8, 64, 128, 33, dy, dx, a, a, ws, None) == -3
    assert L.vqvae_conv_taps_wgrad_f32(a + 4, a, 1, 8, 8, 64, 128, 6, dy, dx, a, a, ws, None) == -3
    assert L.vqvae_conv_taps_wgrad_f32(a, a, 1, 8, 8, 64, 128, 6, dy, dx, a, a, ws - 4, None) == -4
    big = (__import__("ctypes").c_int8 * 6)(-8, -1, -1, 0, 0, 0)
    assert L.vqvae_conv_taps_wgrad_f32(a, a, 1, 8, 8, 64, 128, 6, big, dx, a, a, ws, None) == -3
    assert L.vqvae_conv_taps_pack_dgrad_bytes(6, 64, 128) > 6 * 64 * 128 * 4
    assert L.vqvae_conv_taps_pack_dgrad_bytes(17, 64, 128) == 0
    assert L.vqvae_conv_taps_pack_dgrad_f32(None, 6, 0, 6, dy, dx, 64, 128, a, None) == -1
    assert L.vqvae_conv_taps_pack_dgrad_f32(a, 6, 2, 6, dy, dx, 64, 128, a, None) == -2          # slice beyond the list
    assert L.vqvae_conv_taps_pack_dgrad_f32(a, 6, 0, 6, dy, dx, 64, 126, a, None) == -3
    assert L.vqvae_gated_activation_backward_f32(a, None, None, None, 1, 64, 64, a, None, None, None) == -1
    assert L.vqvae_gated_activation_backward_f32(a, None, None, a, 1, 64, 64, a, None, a, None) == -1   # grad_cond needs cond
    assert L.vqvae_gated_activation_backward_f32(a, None, a, a, 0, 64, 64, a, None, a, None) == -2
    assert L.vqvae_gather_rows_backward_workspace_bytes(0, 64, 512) == 0
    assert L.vqvae_gather_rows_backward_workspace_bytes(256, 64, 512) > 256 * 16
    assert L.vqvae_gather_rows_backward_f32(None, a, 256, 64, 512, a, a, 1 << 30, None) == -1
    assert L.vqvae_gather_rows_backward_f32(a, a, 256, 0, 512, a, a, 1 << 30, None) == -2
    assert L.vqvae_gather_rows_backward_f32(a, a, 256, 64, 512, a, a, 16, None) == -4
    assert L.vqvae_cross_entropy_workspace_bytes(0) == 0
    assert L.vqvae_cross_entropy_f32(a, None, 64, 512, a, a, 1 << 20, None) == -1
    assert L.vqvae_cross_entropy_f32(a, a, 64, 0, a, a, 1 << 20, None) == -2
    assert L.vqvae_cross_entropy_f32(a, a, 64, 512, a, a, 8, None) == -4
    assert L.vqvae_cross_entropy_backward_f32(a, a, 64, 512, None, None, None) == -1
    assert L.vqvae_bias_grad_wide_workspace_bytes(0) == 0
    assert L.vqvae_bias_grad_wide_workspace_bytes(512) > 0
    assert L.vqvae_bias_grad_wide_f32(None, 64, 512, a, a, 1 << 20, None) == -1
    assert L.vqvae_bias_grad_wide_f32(a, 0, 512, a, a, 1 << 20, None) == -2
    assert L.vqvae_bias_grad_wide_f32(a, 64, 512, a, a, 8, None) == -4
    assert L.vqvae_bias_grad_workspace_bytes(512) == 0                     # the narrow entry keeps its C <= 256 contract
    assert L.vqvae_abi_version() == 9


def test_eval_and_no_grad_paths_are_chosen_without_gpu():
    """the switch between the forward-only path and the autograd path (nothing is launched)"""
    from vqvae_amd.pixelcnn import GatedPixelCNN, _autograd_wanted
    m = GatedPixelCNN(16, 8, 2, 3)
    assert _autograd_wanted(m.train())
    assert not _autograd_wanted(m.eval())
    with torch.no_grad():
        assert not _autograd_wanted(m.train())
    m.requires_grad_(False)
    assert not _autograd_wanted(m.train())
