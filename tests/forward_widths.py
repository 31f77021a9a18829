"""Case table and CPU-side helpers of tests/test_forward_widths_gpu.py: the 32x32, h_dim = 128 models whose whole-path plan
(fwd_plan, vqvae_amd/csrc/model.hip) takes the fused 8x8 kernels at widths other than res_h_dim = 32, D = 64.

Every model is VQVAE(128, Rh, nl, K, D, 0.25) built right after torch.manual_seed(0), in eval mode.  Each runs with two codebooks:

  "init"  the constructor's codebook (uniform in +-1/K: z_q entering the decoder is ~1e-3, a handful of codes ever win);
  "data"  rows of the oracle's own z_e on a second batch plus 0.02 * randn: many codes win, z_q is at the scale of z_e.

The inputs are chosen so that the REFERENCE has no row that could flip: the x seeds below are the first in 0..63 for which no row
is fragile (fragile_rows), so the GPU test may assert the indices exactly.  test_no_fragile_row_in_any_case (CPU) recomputes that.

What each row launches is derived from fwd_plan and the entry points behind it, not measured:

  enc_igemm   launches the encoder ENTRY (vqvae_encoder_f32) records under 'conv_igemm': 1 = enc_front8_h2_kernel alone (the 3x3 conv,
              both residual layers and the 1x1 conv are ONE conv_res_pair8_h2_kernel, recorded under 'res_layer'); 3 = enc_front plus
              the 3x3 and the 1x1 conv as layerwise launches (p.enc_pair_post false: D outside {32, 64, 128}, or nl != 2)
  enc_res     launches it records under 'res_layer': 1 = one fused pair (with or without the front conv); nl = 3: a pair and a single
              layer; nl = 1: the single layer
  fwd_res     'res_layer' launches of vqvae_forward_f32's default route: 1 = the quantizing kernel carries the decoder's head
              (p.mid_fuse); 2 = encoder-side kernel + dec_front; nl = 3 / 1: the per-layer residual kernels of both stacks
  vq_fused    the quantizer rides in the encoder's last kernel (p.vq_fuse: D = 64, K <= 1024, ceil(K/32) % 4 == 0): no 'vq_main' launch;
              the VQVAE_FWD_DEBUG_ZE route then records 2 'res_layer' launches (quantizing kernel, dec_front)."""
import collections
import functools
import math

import torch

Case = collections.namedtuple("Case", "Rh nl K D B seed_init seed_data enc_igemm enc_res fwd_res vq_fused")

CASES = {
    # name:              Rh nl    K    D  B  seeds   enc_igemm enc_res fwd_res vq_fused
    "rh16_k512_d64":    Case(16, 2, 512, 64, 5, 0, 0, 1, 1, 1, True),      # three launches, half of the hidden tile padding
    "rh1_k256_d64":     Case(1, 2, 256, 64, 5, 0, 0, 1, 1, 1, True),       # one real hidden channel
    "rh20_k1024_d64":   Case(20, 2, 1024, 64, 5, 1, 2, 1, 1, 1, True),     # Rh not a multiple of 8, eight codebook stages
    "rh31_k100_d64":    Case(31, 2, 100, 64, 9, 3, 0, 1, 1, 1, True),      # padding codes and one padding hidden channel
    "rh32_k512_d32":    Case(32, 2, 512, 32, 5, 1, 0, 1, 1, 2, False),     # post <1>, stand-alone quantizer, front / gather at Cin 32
    "rh8_k100_d32":     Case(8, 2, 100, 32, 5, 0, 1, 1, 1, 2, False),      # the same, narrow
    "rh32_k512_d128":   Case(32, 2, 512, 128, 5, 1, 0, 1, 1, 2, False),    # post <4>, front / gather at Cin 128
    "rh24_k2048_d128":  Case(24, 2, 2048, 128, 3, 2, 0, 1, 1, 2, False),   # the same behind the streamed quantizer
    "rh16_k2048_d64":   Case(16, 2, 2048, 64, 5, 0, 1, 1, 1, 2, False),    # all four fused, quantizer not fused (K > 1024)
    "rh16_k96_d64":     Case(16, 2, 96, 64, 5, 1, 0, 1, 1, 2, False),      # the same (three 32-code groups)
    "rh32_k512_d256":   Case(32, 2, 512, 256, 3, 0, 0, 3, 1, 2, False),    # mixed plan: layerwise encoder middle, dec_front at Cin 256
    "rh12_k300_d96":    Case(12, 2, 300, 96, 5, 0, 0, 3, 1, 2, False),     # mixed plan, three input chunks, any-width quantizer
    "rh16_n3_k512_d64": Case(16, 3, 512, 64, 5, 1, 0, 3, 2, 4, False),     # fused ends only, per-layer residual kernels
    "rh4_n1_k512_d32":  Case(4, 1, 512, 32, 5, 0, 0, 3, 1, 2, False),      # the same
}
CODEBOOKS = ("init", "data")
FUSED_VQ = [n for n, c in CASES.items() if c.vq_fused]
MIXED = ("rh32_k512_d256", "rh12_k300_d96")
BETA = 0.25
SEED_TRIES = 64

E5 = "encoder.conv_stack.5.stack.0.res_block."
D1 = "decoder.inverse_conv_stack.1.stack.0.res_block."
CB = "vector_quantization.embedding.weight"


def model(name):
    """the CPU model of a row, default initialisation"""
    from vqvae_amd.modules import VQVAE
    c = CASES[name]
    torch.manual_seed(0)
    return VQVAE(128, c.Rh, c.nl, c.K, c.D, BETA).eval()


@functools.lru_cache(maxsize=None)
def _init_state(name):
    return {k: v.detach().clone() for k, v in model(name).state_dict().items()}


@functools.lru_cache(maxsize=None)
def _data_codebook(name):
    from oracle import torch_port
    c = CASES[name]
    g = torch.Generator().manual_seed(999)
    xb = torch.randn(max(8, math.ceil(c.K / 64)), 3, 32, 32, generator=g)
    with torch.no_grad():
        rows = torch_port.encode(_init_state(name), xb, c.nl).permute(0, 2, 3, 1).reshape(-1, c.D)[:c.K]
    return (rows + 0.02 * torch.randn(c.K, c.D, generator=g)).contiguous()


def state(name, codebook):
    """a fresh state dict (the caller may change it) of a row with the "init" or the "data" codebook"""
    sd = {k: v.clone() for k, v in _init_state(name).items()}
    if codebook == "data":
        sd[CB] = _data_codebook(name).clone()
    else:
        assert codebook == "init"
    return sd


def inputs(name, seed):
    return torch.randn(CASES[name].B, 3, 32, 32, generator=torch.Generator().manual_seed(seed))


def seed_of(name, codebook):
    c = CASES[name]
    return c.seed_init if codebook == "init" else c.seed_data


def oracle(sd, x, nl):
    """oracle/torch_port.py stage by stage -> dict(z_e (B,D,8,8), z_q, idx (N,1), x_hat, loss, ppl)"""
    from oracle import torch_port
    with torch.no_grad():
        z_e = torch_port.encode(sd, x.clone(), nl)
        loss, z_q, ppl, _, idx = torch_port.quantize(z_e, sd[CB], BETA)
        x_hat = torch_port.decode(sd, z_q.clone(), nl)
    return dict(z_e=z_e, z_q=z_q, idx=idx, x_hat=x_hat, loss=float(loss), ppl=float(ppl))


def fragile_rows(z_e, idx, codebook):
    """Rows of the oracle's z_e (B,D,8,8) whose winner b = idx could lose to another code k, in fp64:

        d_k - d_b <= 8 * 2^-24 * (|z|^2 + max(|e_k|^2, |e_b|^2)) + 4e-6 * ||e_b - e_k||_1

    The first term is the near-tie bound of the other forward tests; the second is what a z_e that is off by the project's
    tolerance (2e-6 per element) can move the gap d_k - d_b = 2 z . (e_b - e_k) + |e_k|^2 - |e_b|^2.  -> the rows' numbers."""
    D = codebook.shape[1]
    z = z_e.permute(0, 2, 3, 1).reshape(-1, D).double()
    e = codebook.double()
    b = idx.view(-1)
    ee = (e * e).sum(1)
    d = (z * z).sum(1, keepdim=True) - 2.0 * z @ e.t() + ee[None, :]     # (expanded, in fp64: its rounding is nine decades below the bound)
    gap = d - d.gather(1, b.view(-1, 1))
    win, inv = torch.unique(b, return_inverse=True)
    l1 = torch.cdist(e[win], e, p=1)[inv]                                   # ||e_b - e_k||_1 for every row's winner
    bound = 8 * 2.0 ** -24 * ((z * z).sum(1, keepdim=True) + torch.maximum(ee[None, :], ee[b][:, None])) + 4e-6 * l1
    bad = gap <= bound
    bad[torch.arange(b.numel()), b] = False
    return torch.nonzero(bad.any(1)).view(-1)


@functools.lru_cache(maxsize=None)
def reference(name, codebook):
    """the oracle's run of a row on its committed x seed; computed once, shared by the tests and never changed by them"""
    sd = state(name, codebook)
    x = inputs(name, seed_of(name, codebook))
    out = oracle(sd, x, CASES[name].nl)
    out.update(sd=sd, x=x)
    return out


def first_clean_seed(name, codebook):
    """the first x seed in 0..63 on which the oracle has no fragile row (how the table's seeds were chosen), or None"""
    sd = state(name, codebook)
    for seed in range(SEED_TRIES):
        o = oracle(sd, inputs(name, seed), CASES[name].nl)
        if fragile_rows(o["z_e"], o["idx"], sd[CB]).numel() == 0:
            return seed
    return None


def scale_last_hidden_channel(sd, Rh, factor=1.0 + 2.0 ** -6):
    """multiply, in place, the raw weights of hidden channel Rh - 1 of both residual stacks: its row of the 3x3 conv and its
    column of the 1x1 conv"""
    for pre in (E5, D1):
        sd[pre + "1.weight"][Rh - 1] *= factor
        sd[pre + "3.weight"][:, Rh - 1] *= factor
