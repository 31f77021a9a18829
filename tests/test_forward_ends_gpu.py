"""GPU tests (-m gpu) of the default 32x32 forward against RECORDED bits: tests/golden/forward_ends.npz holds x_hat, embedding_loss,
perplexity and the indices that the library of the commit before the end kernels' staged tables computed (enc_front8_h2_kernel /
dec_tail8_h2_kernel read their biases and per-channel scales from tables staged on chip: where the values come from changes, not the
operands or their order per accumulator).  Every output must be identical BIT FOR
BIT; there is no tolerance in this file.

The cases and the construction of model and input are those of tools/gen_golden_forward_ends.py (which wrote the fixture, with the
earlier library): B in {1, 4, 5, 9} x K in {256, 512} -- idle waves, one full workgroup, a partial last workgroup -- and the biases of
the first two and the last two layers as zero tensors and at |b| ~ 10.  Borders and scale extremes of the two kernels are pinned by
tests/test_model_gpu.py (test_encoder_front_fusion_scales_and_borders / test_decoder_tail_fusion_scales_and_borders)."""
import os

import numpy as np
import pytest
import torch

from tools import gen_golden_forward_ends as gen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_ends.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_case(golden):
    for name, B, K, _ in gen.CASES:
        assert golden[f"{name}/x_hat"].shape == (B, 3, 32, 32) and golden[f"{name}/x_hat"].dtype == np.uint32
        assert golden[f"{name}/idx"].shape == (B * 64,) and 0 <= golden[f"{name}/idx"].min() and golden[f"{name}/idx"].max() < K


@pytest.mark.parametrize("name,B,K,bias_mode", gen.CASES, ids=[c[0] for c in gen.CASES])
def test_same_bits_as_recorded(golden, name, B, K, bias_mode):
    got = gen.run_case(name, B, K, bias_mode, torch.device("cuda:0"))
    # the same model and images as the generator had (else: another torch generator / initialisation, not another kernel)
    assert str(got["inputs"]) == str(golden[f"{name}/inputs"]), f"{name}: model parameters or input images differ from the recorded run's"
    if bias_mode == "large":
        m = gen.make_model(K, bias_mode, torch.device("cpu"))
        for n in gen.END_BIASES:
            b = dict(m.named_parameters())[n].detach().abs()
            assert 8.0 <= float(b.min()) and float(b.max()) <= 12.0
    want_idx, want_x = golden[f"{name}/idx"], golden[f"{name}/x_hat"]
    assert np.array_equal(got["idx"], want_idx), f"{name}: {int((got['idx'] != want_idx).sum())} of {want_idx.size} indices differ"
    assert np.array_equal(got["x_hat"], want_x), f"{name}: {int((got['x_hat'] != want_x).sum())} of {want_x.size} x_hat elements differ in their bits"
    for what in ("loss", "perplexity"):
        assert np.array_equal(got[what], golden[f"{name}/{what}"]), \
            f"{name}: {what} {got[what].view(np.float32)[0]!r} vs recorded {golden[f'{name}/{what}'].view(np.float32)[0]!r}"
