"""Host-side mirror of the reference's module interface for the forward hot path.

Same class names, constructor signatures, attribute names, parameter names/shapes
and `state_dict` layout as the reference, so checkpoints written by
the reference (`utils.py:109-113`) load unchanged and callers (`main.py:74`,
`visualization.ipynb:84-90`) keep working:

    VQVAE(h_dim, res_h_dim, n_res_layers, n_embeddings, embedding_dim, beta,
          save_img_embedding_map=False).forward(x) -> (embedding_loss, x_hat, perplexity)
                                                              (models/vqvae.py:11-12,29-44)
    VectorQuantizer(n_e, e_dim, beta).forward(z)
          -> (loss, z_q, perplexity, min_encodings, min_encoding_indices)   (models/quantizer.py:20,29-76)
    Encoder(in_dim, h_dim, n_res_layers, res_h_dim)                          (models/encoder.py:24)
    Decoder(in_dim, h_dim, n_res_layers, res_h_dim)                          (models/decoder.py:22)
    ResidualLayer(in_dim, h_dim, res_h_dim), ResidualStack(in_dim, h_dim, res_h_dim, n_res_layers)
                                                                             (models/residual.py:16,41)

The modules only HOLD parameters; the arithmetic is libvqvae_hip.so, on CUDA(HIP)
fp32 tensors only -- there is no CPU fallback.  `VQVAE.forward` under autograd (main.py:74-79) runs every
layer forward and backward on the HIP kernels (autograd_conv.py, training.VQStraightThrough; SURVEY.md 8f
row 2).  The sub-modules called on their own (`Encoder`, `Decoder`, `ResidualStack`) are forward-only on the
HIP backend and raise while a graph is being recorded.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _cache
from . import functional as F_hip
from ._lib import VqvaeHipError


def _records_graph(*tensors):
    """Is a graph being recorded through the HIP conv path?  (round 5: the sub-modules then run autograd_conv's Functions --
    forward AND backward on the HIP kernels -- as VQVAE.forward does; models/encoder.py:42-43, decoder.py:38-39,
    residual.py:47-51 are differentiable upstream, and so are they here)"""
    from . import conv as C_hip
    return C_hip.get_conv_backend() == "hip" and torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _require_forward_only(*tensors):
    """The whole-path / fused forward entries keep no activations: refuse to run them while a graph is recorded."""
    if _records_graph(*tensors):
        raise VqvaeHipError(
            "this entry point is forward-only: call it under torch.no_grad() (or model.requires_grad_(False)); "
            "VQVAE.forward, Encoder / Decoder / ResidualStack.forward record a graph on the HIP kernels by themselves.  "
            "There is no silent fallback")


def _need_hip_f32(x, who):
    if not x.is_cuda or x.dtype != torch.float32:
        raise VqvaeHipError(f"{who} needs a CUDA(HIP) fp32 input: there is no CPU path")


class LazyOneHot:
    """`min_encodings` of VectorQuantizer.forward (models/quantizer.py:55-57): the (N, K) fp32 one-hot -- 512 MiB at BASELINE config
    3's size, 128 GiB at config 5's -- which neither caller of the reference reads (models/vqvae.py:34 and visualization.ipynb:87
    both discard it).  SURVEY.md 8b: materialise lazily.  This stands in the return tuple, knows its shape / dtype / device, and
    becomes the real tensor (vqvae_vq_onehot_f32, once) the moment anything is done with it: attribute access, indexing, arithmetic,
    or being passed to a torch function.  `VectorQuantizer.LAZY_MIN_ENCODINGS = False` returns the tensor itself as before."""

    def __init__(self, idx, n_e):
        # its own copy: the caller also gets `idx` (the fifth output) and may edit it in place before the one-hot is first used
        self._idx, self._n_e, self._t = idx.clone(), n_e, None

    def materialize(self):
        if self._t is None:
            self._t = F_hip.vq_onehot(self._idx, self._n_e)
        return self._t

    @property
    def shape(self):
        return torch.Size((self._idx.shape[0], self._n_e))

    @property
    def dtype(self):
        return torch.float32

    @property
    def device(self):
        return self._idx.device

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return 2

    def numel(self):
        return self._idx.shape[0] * self._n_e

    def __len__(self):
        return self._idx.shape[0]

    def __getattr__(self, name):                      # anything else: the tensor's
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        def real(a):
            if isinstance(a, LazyOneHot):
                return a.materialize()
            if isinstance(a, (list, tuple)):
                return type(a)(real(v) for v in a)
            return a
        return func(*real(args), **{k: real(v) for k, v in (kwargs or {}).items()})

    def __repr__(self):
        return f"LazyOneHot(shape={tuple(self.shape)}, materialized={self._t is not None})"


def _delegate(name):
    def op(self, *a, **k):
        return getattr(self.materialize(), name)(*[v.materialize() if isinstance(v, LazyOneHot) else v for v in a], **k)
    op.__name__ = name
    return op


for _n in ("__getitem__", "__iter__", "__add__", "__radd__", "__sub__", "__rsub__", "__mul__", "__rmul__", "__truediv__", "__matmul__",
           "__rmatmul__", "__eq__", "__ne__", "__lt__", "__le__", "__gt__", "__ge__", "__neg__", "__bool__", "__float__", "__int__",
           "__array__"):
    setattr(LazyOneHot, _n, _delegate(_n))
LazyOneHot.__hash__ = object.__hash__


class VectorQuantizer(nn.Module):
    """Discretisation bottleneck; mirrors models/quantizer.py:10-76."""

    LAZY_MIN_ENCODINGS = True          # forward()'s fourth output: LazyOneHot (the (N, K) one-hot on first use) or the tensor itself

    def __init__(self, n_e, e_dim, beta, *, rotation_trick=False, cosine_sim=False, orthogonal_reg_weight=0.0,
                 orthogonal_reg_active_codes_only=False, orthogonal_reg_max_codes=None, generator=None, entropy_weight=0.0,
                 entropy_diversity_gamma=1.0, entropy_inv_temperature=100.0):
        super().__init__()
        self.n_e = n_e
        self.e_dim = e_dim
        self.beta = beta
        # opt-in: the code-entropy loss (MaskGIT's VQGAN tokenizer, MAGVIT, LlamaGen's `entropy_loss_ratio`; csrc/vq_entropy.hip) joins
        # the training loss: weight * (P - gamma * H) of the rows' softmax over the codes at -inv_temperature * squared distance.  On
        # unit rows d = 2 - 2 cos, so inv_temperature = 50 with cosine_sim is MaskGIT's temperature of 0.01.  Plain attributes: no
        # parameter, no buffer, no state_dict key; at weight 0 nothing is launched.
        self.entropy_weight, self.entropy_diversity_gamma, self.entropy_inv_temperature = self._check_entropy(
            entropy_weight, entropy_diversity_gamma, entropy_inv_temperature)
        self.last_entropy_losses = None        # the latest (term, P, H), a device 3-vector
        # opt-in: the orthogonal regularization loss of the codebook (arXiv 2112.00384 section 3.2; csrc/vq_orthogonal.hip) joins
        # the training loss.  Plain attributes: no parameter, no buffer, no state_dict key; at weight 0 nothing is launched or drawn.
        self.orthogonal_reg_weight, self.orthogonal_reg_max_codes = self._check_orthogonal(orthogonal_reg_weight,
                                                                                           orthogonal_reg_max_codes)
        self.orthogonal_reg_active_codes_only = bool(orthogonal_reg_active_codes_only)
        self.generator = generator             # of the cap's draws (VectorQuantizerEMA: of its restart rows)
        self.last_orthogonal_loss = None       # the latest term, a device scalar
        # opt-in: the decoder's gradient reaches the encoder through the rotation trick (arXiv 2410.06424; csrc/vq_rotation.hip)
        # instead of unchanged.  A plain attribute: no parameter, no buffer, no state_dict key; the forward is the same.
        self.rotation_trick = bool(rotation_trick)
        # opt-in: the cosine-similarity codebook (ViT-VQGAN, arXiv 2110.04627 section 3.2; csrc/vq_cosine.hip): z and the codes are
        # l2-normalised, then quantized exactly as without the option.  A plain attribute too; `embedding.weight` is stored
        # un-normalised and normalised on use.
        self.cosine_sim = bool(cosine_sim)
        self.embedding = nn.Embedding(self.n_e, self.e_dim)
        self.embedding.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)   # quantizer.py:27

    @staticmethod
    def _check_orthogonal(weight, max_codes):
        weight = float(weight)
        if not weight >= 0.0:
            raise ValueError(f"orthogonal_reg_weight must be >= 0, got {weight!r}")
        if max_codes is not None:
            if isinstance(max_codes, bool) or not isinstance(max_codes, int) or max_codes < 1:
                raise ValueError(f"orthogonal_reg_max_codes must be an int >= 1 or None, got {max_codes!r}")
        return weight, max_codes

    @staticmethod
    def _check_entropy(weight, gamma, inv_temperature):
        weight, gamma, inv_temperature = float(weight), float(gamma), float(inv_temperature)
        if not weight >= 0.0 or weight == float("inf"):
            raise ValueError(f"entropy_weight must be >= 0 and finite, got {weight!r}")
        if not (inv_temperature > 0.0 and inv_temperature < float("inf")):
            raise ValueError(f"entropy_inv_temperature must be > 0 and finite, got {inv_temperature!r}")
        if gamma != gamma or abs(gamma) == float("inf"):
            raise ValueError(f"entropy_diversity_gamma must be finite, got {gamma!r}")
        return weight, gamma, inv_temperature

    def _with_entropy(self, out, z, codes, rowmajor):
        """quantize's outputs with entropy_weight * the code-entropy term added to the loss: only with a weight > 0, in training
        mode, while a graph is recorded.  z, codes: the very operands the search ran on -- the unit rows and unit codes with
        cosine_sim, the projected rows and the low-dimensional codebook with codebook_dim.  A codebook that takes no gradient (EMA)
        is passed without one: only z gets a gradient.  (term, P, H) is kept in last_entropy_losses."""
        if not (self.entropy_weight > 0.0 and self.training and torch.is_grad_enabled() and (z.requires_grad or codes.requires_grad)):
            return out
        from .training import CodeEntropyLoss
        if not codes.requires_grad and codes.data_ptr() == self.embedding.weight.data_ptr():
            codes = codes.detach().clone()     # an EMA update writes embedding.weight in place before the backward reads the codes
        N = out[3].numel()
        table = _cache.side(self).setdefault("entropy_ws", {})
        skey = (str(z.device), torch.cuda.current_stream(z.device).cuda_stream, N)
        ws = _cache.lru_get(table, skey)
        if ws is None:
            ws = F_hip.vq_entropy_workspace(N, self.n_e, self.e_dim, z.device)
            _cache.lru_put(table, skey, ws, 4)
        term = CodeEntropyLoss.apply(z, codes, self.entropy_inv_temperature, self.entropy_diversity_gamma, rowmajor, ws)
        self.last_entropy_losses = CodeEntropyLoss.last_losses
        return (out[0] + self.entropy_weight * term,) + tuple(out[1:])

    def _with_orthogonal(self, out, codes):
        """quantize's outputs with weight * the orthogonal regularization loss of the l2-normalised codebook added to the loss:
        only with a weight > 0, in training mode, while a graph is recorded, for a codebook that takes a gradient.  codes: the
        rows the search ran on -- with cosine_sim the normalised codebook's node, which is used as it is (the codebook is
        normalised once).  The term is kept in last_orthogonal_loss."""
        w = self.embedding.weight
        if not (self.orthogonal_reg_weight > 0.0 and self.training and torch.is_grad_enabled() and w.requires_grad):
            return out
        from .training import L2NormRows, OrthogonalLoss
        unit = codes if self.cosine_sim else L2NormRows.apply(w)
        table = _cache.side(self).setdefault("orth_ws", {})
        skey = (str(w.device), torch.cuda.current_stream(w.device).cuda_stream)
        ws = _cache.lru_get(table, skey)
        if ws is None:
            ws = F_hip.vq_orthogonal_workspace(self.n_e, self.e_dim, w.device)
            _cache.lru_put(table, skey, ws, 8)
        max_codes, uniforms = self.orthogonal_reg_max_codes, None
        if max_codes is not None:
            uniforms = torch.rand(self.n_e, device=w.device, generator=self.generator)
        term = OrthogonalLoss.apply(unit, out[4] if self.orthogonal_reg_active_codes_only else None, max_codes, uniforms, ws)
        self.last_orthogonal_loss = term.detach()
        return (out[0] + self.orthogonal_reg_weight * term,) + tuple(out[1:])

    def invalidate(self):
        """Forget the prepared codebook image.  The cache is keyed on (data_ptr, _version, device), which in-place ops
        and optimizers bump; writes through `.data` (`weight.data.copy_()`, EMA updates) do NOT -- call this after
        such a write.  `load_state_dict` and `.to()/.cuda()` call it for you."""
        for slot in _cache.side(self).get("ws", {}).values():
            slot[1] = None
        _cache.drop(self, "cosine_codebook")

    def _codebook_key(self):
        w = self.embedding.weight
        # (with cosine_sim the prepared image is the normalised codebook's: flipping the attribute re-keys)
        return (w.data_ptr(), w._version, w.device) + (("cosine",) if self.cosine_sim else ())

    def normalized_codebook(self):
        """The l2-normalised codebook (K, D) that a cosine_sim quantizer searches and decodes with, without grad: computed once per
        version of `embedding.weight` (keyed as the prepared codebook image is; invalidate() drops it)."""
        w = self.embedding.weight
        key = (w.data_ptr(), w._version, w.device)
        hit = _cache.side(self).get("cosine_codebook")
        if hit is None or hit[0] != key:
            hit = (key, F_hip.l2norm_rows(w.detach())[0])
            _cache.side(self)["cosine_codebook"] = hit
        return hit[1]

    def _cosine_operands(self, z, rowmajor):
        """-> (z^, E^): the rows the quantizer runs on with cosine_sim.  While a graph is recorded both go through L2NormRows (the
        gradients of z and of the codebook pass through the normalisation's backward); otherwise functional.l2norm_rows and the
        cached E^."""
        w = self.embedding.weight
        if torch.is_grad_enabled() and (z.requires_grad or w.requires_grad):
            from .training import L2NormRows
            return L2NormRows.apply(z, rowmajor), (L2NormRows.apply(w) if w.requires_grad else self.normalized_codebook())
        return F_hip.l2norm_rows(z, rowmajor=rowmajor)[0], self.normalized_codebook()

    def _workspace(self):
        """-> (workspace, prepared, key, slot): workspace holding the codebook's LDS images and the per-call scratch,
        ONE PER (device, stream) -- two forwards of one model on different streams must not share scratch -- re-prepared
        only when the embedding tensor changes.  The caller stores `key` in slot[1] once the launch has succeeded."""
        w = self.embedding.weight
        key = self._codebook_key()
        table = _cache.side(self).setdefault("ws", {})
        skey = (str(w.device), torch.cuda.current_stream(w.device).cuda_stream if w.is_cuda else 0)
        slot = _cache.lru_get(table, skey)
        if slot is None:
            slot = [F_hip.vq_workspace(self.n_e, self.e_dim, w.device), None]
            _cache.lru_put(table, skey, slot, 8)                 # streams come and go: the least recently used slot leaves
        return slot[0], slot[1] == key, key, slot

    def quantize(self, z, *, rowmajor=False, want_zq=True):
        """-> (loss, z_q, perplexity, min_encoding_indices, hist); no one-hot."""
        w = self.embedding.weight
        ws, prepared, key, slot = self._workspace()
        if not prepared:
            slot[1] = None                                       # a failed launch must not leave a stale "prepared" image
        if self.cosine_sim:
            z, w = self._cosine_operands(z, rowmajor)            # from here on: today's quantizer, on the unit rows
        if torch.is_grad_enabled() and (z.requires_grad or w.requires_grad):
            from .training import VQStraightThrough          # HIP forward + HIP backward
            out = VQStraightThrough.apply(z, w, self.beta, rowmajor, ws, prepared, self.rotation_trick)
        else:
            out = F_hip.vq_forward(z, w.detach(), self.beta, rowmajor=rowmajor, workspace=ws,
                                   prepared=prepared, want_zq=want_zq)
        slot[1] = key
        return self._with_entropy(self._with_orthogonal(out, w), z, w, rowmajor)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    @torch.no_grad()
    def init_codebook_(self, z, iters=10, generator=None, *, rowmajor=False):
        """Opt-in data-dependent start: the codebook becomes k-means (k-means++ seeding and `iters` Lloyd rounds on the HIP kernels,
        functional.vq_kmeans) of the rows of z -- encoder outputs (B,D,H,W), or (B,H,W,D) when rowmajor -- instead of
        uniform(-1/K, 1/K).  Written into `embedding.weight` by an in-place op: its `_version` moves, so the prepared and packed
        codebook images re-key.  cosine_sim: k-means of the l2-normalised rows (spherical k-means; the centroids are stored as
        they come and normalised on use).  -> (codebook, counts of the last assignment)."""
        _need_hip_f32(z, "init_codebook_")
        if self.cosine_sim:
            z = F_hip.l2norm_rows(z.detach(), rowmajor=rowmajor)[0]
        codebook, counts = F_hip.vq_kmeans(z.detach(), self.n_e, iters, generator=generator, rowmajor=rowmajor)
        self.embedding.weight.copy_(codebook)
        return codebook, counts

    def forward(self, z):
        loss, z_q, perplexity, idx, _ = self.quantize(z)
        min_encodings = LazyOneHot(idx, self.n_e) if self.LAZY_MIN_ENCODINGS else F_hip.vq_onehot(idx, self.n_e)   # quantizer.py:55-57
        return loss, z_q, perplexity, min_encodings, idx


def _drop_pending_after_load(module, incompatible_keys):
    """load_state_dict post-hook of an EMA quantizer with sync / accumulate (a module-level function: it must pickle)."""
    _cache.drop(module, "ema_pending")


class _EMAMerge:
    """What the EMA quantizers share for `sync` / `accumulate`: instead of one update per training forward, a forward takes one
    record of sufficient statistics per codebook (functional.vq_ema_stats) into a pending device buffer (A, G, K, C); on the A-th
    record the records -- with `sync` and an initialised process group of W > 1 ranks, the records of every rank, rank-major --
    are applied once (functional.vq_ema_apply, R = A or W A shards added in a fixed order) and the new codebooks are copied into
    the parameters in place.  G: the codebooks of the module (1, or the groups).  Forwards inside a cycle all see one codebook.

    The pending records live in the weak side table (never in the state_dict): load_state_dict, invalidate(), .to() and
    init_codebook_ drop them.  The collectives are reached through `_ema_gather` and `_ema_broadcast`, which an instance may
    replace (the defaults are sharding.all_gather_ema_stats and sharding.broadcast_ema_uniforms).

    Restart: one torch.rand(2, K) per codebook, in group order, at the first record of a cycle, from `generator` or the default
    CUDA generator; under `sync` overwritten by rank 0's.  Row 0 picks the shard (shard_uniforms), row 1 the row of every shard
    (every record's row_uniforms).  Without a threshold nothing is drawn or broadcast."""

    @staticmethod
    def _ema_gather(stats, group=None):
        from . import sharding
        return sharding.all_gather_ema_stats(stats, group)

    @staticmethod
    def _ema_broadcast(u, group=None):
        from . import sharding
        return sharding.broadcast_ema_uniforms(u, group)

    @staticmethod
    def _check_accumulate(accumulate):
        if isinstance(accumulate, bool) or not isinstance(accumulate, int) or not 1 <= accumulate <= 1024:
            raise ValueError(f"accumulate must be an int in [1, 1024], got {accumulate!r}")
        return accumulate

    def _init_ema_merge(self, sync, accumulate):
        self.ema_sync = bool(sync)
        self.ema_accumulate = self._check_accumulate(accumulate)
        if self._ema_merging:
            self.register_load_state_dict_post_hook(_drop_pending_after_load)

    @property
    def _ema_merging(self):
        return self.ema_sync or self.ema_accumulate > 1

    @property
    def pending_ema_updates(self) -> int:
        """records taken since the last apply"""
        pend = _cache.side(self).get("ema_pending")
        return pend["count"] if pend else 0

    def _ema_states(self):
        """[(ema_cluster_size (K,), ema_w (K, d), codebook parameter)] in group order"""
        return [(self.ema_cluster_size, self.ema_w, self.embedding.weight)]

    def _ema_side_ws(self, name, key, make):
        table = _cache.side(self).setdefault(name, {})
        ws = _cache.lru_get(table, key)
        if ws is None:
            ws = make()
            _cache.lru_put(table, key, ws, 4)
        return ws

    def _ema_record(self, zs, idxs, rowmajor):
        """one record per codebook from this forward's rows zs[g] and indices idxs[g]; the A-th record applies"""
        states = self._ema_states()
        w = states[0][2]
        dev, (K, d), G, A = w.device, w.shape, len(states), self.ema_accumulate
        restart = self.restart_threshold is not None
        C = 2 * d + 1 if restart else d + 1
        side = _cache.side(self)
        pend = side.get("ema_pending")
        if pend is None or pend["buf"].shape != (A, G, K, C) or pend["buf"].device != dev:
            pend = side["ema_pending"] = {"count": 0, "uniforms": None,
                                          "buf": torch.empty((A, G, K, C), dtype=torch.float64, device=dev)}
        if pend["count"] == 0 and restart:
            u = torch.stack([torch.rand(2, K, device=dev, generator=self.generator) for _ in range(G)])
            if self.ema_sync:
                got = self._ema_broadcast(u)
                u = u if got is None else got
            pend["uniforms"] = u
        u = pend["uniforms"]
        N = idxs[0].numel()
        ws = self._ema_side_ws("ema_stats_ws", (str(dev), torch.cuda.current_stream(dev).cuda_stream, N),
                               lambda: F_hip.vq_ema_stats_workspace(N, K, d, dev))
        a = pend["count"]
        for g in range(G):
            F_hip.vq_ema_stats(zs[g], idxs[g], K, row_uniforms=u[g, 1] if restart else None, rowmajor=rowmajor, workspace=ws,
                               out=pend["buf"][a, g])
        pend["count"] = a + 1
        if pend["count"] >= A:
            self.flush_ema_()

    @torch.no_grad()
    def flush_ema_(self):
        """Apply what is pending now, with R = pending (W * pending under `sync` with W > 1 ranks: every rank must then hold the
        same number of records), and start a new cycle.  Nothing pending: nothing happens."""
        pend = _cache.side(self).get("ema_pending")
        if not pend or pend["count"] == 0:
            return
        A, (_, G, K, C) = pend["count"], pend["buf"].shape
        stats = pend["buf"][:A].reshape(A, G * K, C)
        if self.ema_sync:
            stats = self._ema_gather(stats)
        R = stats.shape[0]
        stats = stats.reshape(R, G, K, C)
        dev = stats.device
        restart = self.restart_threshold is not None
        u = pend["uniforms"]
        states = self._ema_states()
        d = states[0][2].shape[1]
        ws = self._ema_side_ws("ema_apply_ws", (str(dev), torch.cuda.current_stream(dev).cuda_stream, R),
                               lambda: F_hip.vq_ema_apply_workspace(R, K, d, dev))
        for g, (cluster_size, ema_w, w) in enumerate(states):
            new = torch.empty_like(w, memory_format=torch.contiguous_format)
            F_hip.vq_ema_apply(stats[:, g], cluster_size, ema_w, new, self.decay, self.eps,
                               threshold=self.restart_threshold, shard_uniforms=u[g, 0] if restart else None, workspace=ws)
            w.copy_(new)
        pend["count"] = 0
        pend["uniforms"] = None


class VectorQuantizerEMA(_EMAMerge, VectorQuantizer):
    """VectorQuantizer whose codebook follows exponential moving averages of the encoder outputs assigned to each code
    (arXiv 1711.00937 Appendix A.1; Sonnet's VectorQuantizerEMA) instead of a gradient.

    State: `embedding.weight` (a Parameter with requires_grad=False: the codebook, same state_dict key and whole-path packing as
    VectorQuantizer), and the buffers `ema_cluster_size` (K,) = N_k (initially 0) and `ema_w` (K, D) = m_k (initially the initial
    codebook).  Every forward in training mode -- with or without grad -- runs one update (vqvae_vq_ema_update_f32) from that
    forward's z and indices, then copies the new codebook into `embedding.weight` in place (its `_version` moves, so every cache
    keyed on it re-keys).  Eval mode never updates.  The forward's outputs are those of the codebook BEFORE the update; the loss
    is the commitment term only, beta * mean((z_q - z)^2), and the codebook gets no gradient.

    restart_threshold: codes whose N_k falls below it take a row of the batch instead (row floor(u_k N), u drawn on the device from
    `generator`, or the default CUDA generator, on every update).  None: no restart.

    sync / accumulate (_EMAMerge): with the defaults every replica of a data-parallel run updates from its own shard after every
    forward.  accumulate=A applies once per A training forwards, from the merged statistics of the A batches; sync=True merges
    the statistics of all ranks of the initialised process group first (every rank must run the same number of training
    forwards), after which all ranks hold bit-identical `embedding.weight`, `ema_cluster_size` and `ema_w`.  `pending_ema_updates`
    counts the records of the open cycle and `flush_ema_()` applies them early."""

    def __init__(self, n_e, e_dim, beta, decay=0.99, eps=1e-5, restart_threshold=None, generator=None, *, rotation_trick=False,
                 cosine_sim=False, entropy_weight=0.0, entropy_diversity_gamma=1.0, entropy_inv_temperature=100.0, sync=False,
                 accumulate=1):
        super().__init__(n_e, e_dim, beta, rotation_trick=rotation_trick, cosine_sim=cosine_sim, entropy_weight=entropy_weight,
                         entropy_diversity_gamma=entropy_diversity_gamma, entropy_inv_temperature=entropy_inv_temperature)
        self.decay = float(decay)
        self.eps = float(eps)
        self.restart_threshold = None if restart_threshold is None else float(restart_threshold)
        self.generator = generator
        self.embedding.weight.requires_grad_(False)
        self.register_buffer("ema_cluster_size", torch.zeros(n_e))
        self.register_buffer("ema_w", self.embedding.weight.detach().clone())
        self._init_ema_merge(sync, accumulate)

    def invalidate(self):
        """VectorQuantizer.invalidate, and the pending statistics of an open sync / accumulate cycle are dropped."""
        super().invalidate()
        _cache.drop(self, "ema_pending")

    def _ema_update(self, z, idx, rowmajor):
        if self._ema_merging:
            return self._ema_record([z], [idx], rowmajor)
        w = self.embedding.weight
        side = _cache.side(self)
        N = idx.numel()
        wkey = (str(w.device), torch.cuda.current_stream(w.device).cuda_stream, N)
        table = side.setdefault("ema_ws", {})
        ws = _cache.lru_get(table, wkey)
        if ws is None:
            ws = F_hip.vq_ema_workspace(N, self.n_e, self.e_dim, w.device)
            _cache.lru_put(table, wkey, ws, 4)
        uniforms = None
        if self.restart_threshold is not None:
            uniforms = torch.rand(self.n_e, device=w.device, generator=self.generator)
        new = torch.empty_like(w, memory_format=torch.contiguous_format)
        F_hip.vq_ema_update(z, idx, self.ema_cluster_size, self.ema_w, new, self.decay, self.eps,
                            threshold=self.restart_threshold, uniforms=uniforms, rowmajor=rowmajor, workspace=ws)
        with torch.no_grad():
            w.copy_(new)

    @torch.no_grad()
    def init_codebook_(self, z, iters=10, generator=None, *, rowmajor=False):
        """VectorQuantizer.init_codebook_, and the EMA state continues from the clusters: ema_cluster_size = counts,
        ema_w = counts[:, None] * codebook."""
        codebook, counts = super().init_codebook_(z, iters, generator, rowmajor=rowmajor)
        _cache.drop(self, "ema_pending")
        c = counts.to(torch.float32)
        self.ema_cluster_size.copy_(c)
        self.ema_w.copy_(c[:, None] * codebook)
        return codebook, counts

    def quantize(self, z, *, rowmajor=False, want_zq=True):
        """-> (beta * mse, z_q, perplexity, min_encoding_indices, hist) against the codebook as it was on entry; then, in training
        mode, one EMA update of the codebook.  cosine_sim: all of it on the l2-normalised rows z^ and codes E^ -- the update runs
        from z^ (restart rows are rows of z^), `embedding.weight` holds ema_w / N_k as without the option and is normalised on use."""
        w = self.embedding.weight
        ws, prepared, key, slot = self._workspace()
        if not prepared:
            slot[1] = None
        if self.cosine_sim:
            z, w = self._cosine_operands(z, rowmajor)
        if torch.is_grad_enabled() and z.requires_grad:
            from .training import VQEMAStraightThrough      # HIP forward + HIP commitment-only backward
            out = VQEMAStraightThrough.apply(z, w, self.beta, rowmajor, ws, prepared, self.rotation_trick)
        else:
            mse, z_q, perplexity, idx, hist = F_hip.vq_forward(z, w.detach(), 0.0, rowmajor=rowmajor, workspace=ws,
                                                               prepared=prepared, want_zq=want_zq)
            out = (mse * self.beta, z_q, perplexity, idx, hist)
        slot[1] = key
        out = self._with_entropy(out, z, w.detach(), rowmajor)     # against the codebook as it was on entry; only z takes a gradient
        if self.training:
            self._ema_update(z.detach(), out[3], rowmajor)
        return out


class FactorizedVectorQuantizer(VectorQuantizer):
    """VectorQuantizer with factorized (low-dimensional) codes (ViT-VQGAN, arXiv 2110.04627 section 3.2; `codebook_dim` in
    vector-quantize-pytorch): a latent row of `dim` channels is projected to `codebook_dim` channels (`project_in`), the codebook is
    searched in that small space, and the chosen code is projected back to `dim` channels (`project_out`).  The quantizer in between
    is VectorQuantizer as it stands, on narrower rows (e_dim = codebook_dim), with every option it has; the loss and the perplexity
    are its own -- the loss is taken in the low-dimensional space.  Both projections run on the HIP kernels of csrc/vq_linear.hip.

    State: `embedding.weight` (n_e, codebook_dim), `project_in` = nn.Linear(dim, codebook_dim), `project_out` =
    nn.Linear(codebook_dim, dim), and nothing else.  Drawn in this order: the codebook, uniform(-1/K, 1/K) as VectorQuantizer draws
    it; then project_in; then project_out (both as nn.Linear initialises itself)."""

    _INNER = VectorQuantizer                  # the class whose quantize / init_codebook_ run on the projected rows

    def __init__(self, n_e, dim, codebook_dim, beta, *, rotation_trick=False, cosine_sim=False, orthogonal_reg_weight=0.0,
                 orthogonal_reg_active_codes_only=False, orthogonal_reg_max_codes=None, generator=None, entropy_weight=0.0,
                 entropy_diversity_gamma=1.0, entropy_inv_temperature=100.0):
        dim, codebook_dim = self._check_dims(dim, codebook_dim)
        super().__init__(n_e, codebook_dim, beta, rotation_trick=rotation_trick, cosine_sim=cosine_sim,
                         orthogonal_reg_weight=orthogonal_reg_weight,
                         orthogonal_reg_active_codes_only=orthogonal_reg_active_codes_only,
                         orthogonal_reg_max_codes=orthogonal_reg_max_codes, generator=generator, entropy_weight=entropy_weight,
                         entropy_diversity_gamma=entropy_diversity_gamma, entropy_inv_temperature=entropy_inv_temperature)
        self._init_projections(dim, codebook_dim)

    @staticmethod
    def _check_dims(dim, codebook_dim):
        for name, v in (("dim", dim), ("codebook_dim", codebook_dim)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 256:
                raise ValueError(f"{name} must be an int in [1, 256], got {v!r}")
        return dim, codebook_dim

    def _init_projections(self, dim, codebook_dim):
        self.dim, self.codebook_dim = dim, codebook_dim
        self.project_in = nn.Linear(dim, codebook_dim)
        self.project_out = nn.Linear(codebook_dim, dim)

    def invalidate(self):
        """VectorQuantizer.invalidate, and the decoded codebook of codebook() is forgotten too."""
        super().invalidate()
        _cache.drop(self, "factorized_codebook")

    @staticmethod
    def _project(x, lin, rowmajor):
        """lin on every row of x: LinearRows while a graph is recorded (x, the weight and the bias get their gradients from the HIP
        backward), functional.linear_rows otherwise"""
        w, b = lin.weight, lin.bias
        if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad):
            from .training import LinearRows
            return LinearRows.apply(x, w, b, rowmajor)
        return F_hip.linear_rows(x, w.detach(), b.detach(), rowmajor=rowmajor)

    def quantize(self, z, *, rowmajor=False, want_zq=True):
        """-> (loss, z_q, perplexity, min_encoding_indices, hist): y = project_in(z); the inner quantizer's quantize of y, in the same
        layout (with EMA: its update from y, or y^ with cosine_sim, in training mode); z_q = project_out of its z_q (None without
        want_zq where no graph is recorded)."""
        _need_hip_f32(z, type(self).__name__)
        y = self._project(z, self.project_in, rowmajor)
        loss, zq_low, perplexity, idx, hist = self._INNER.quantize(self, y, rowmajor=rowmajor, want_zq=want_zq)
        z_q = self._project(zq_low, self.project_out, rowmajor) if zq_low is not None else None
        return loss, z_q, perplexity, idx, hist

    @torch.no_grad()
    def codes(self):
        """the (K, codebook_dim) table that is searched: `embedding.weight`, l2-normalised with cosine_sim"""
        return self.normalized_codebook() if self.cosine_sim else self.embedding.weight.detach()

    @torch.no_grad()
    def codebook(self):
        """the (K, dim) decoded rows project_out(codes()): what decode_indices gathers from.  Computed once per (data_ptr, _version)
        of `embedding.weight`, `project_out.weight` and `project_out.bias`; invalidate() (after a write through `.data`) and
        .to() / .cuda() drop it."""
        ts = (self.embedding.weight, self.project_out.weight, self.project_out.bias)
        _need_hip_f32(ts[0], type(self).__name__ + ".codebook")
        key = tuple((t.data_ptr(), t._version) for t in ts) + (ts[0].device, self.cosine_sim)
        hit = _cache.side(self).get("factorized_codebook")
        if hit is None or hit[0] != key:
            hit = (key, F_hip.linear_rows(self.codes(), ts[1].detach(), ts[2].detach()))
            _cache.side(self)["factorized_codebook"] = hit
        return hit[1]

    @torch.no_grad()
    def init_codebook_(self, z, iters=10, generator=None, *, rowmajor=False):
        """The inner quantizer's init_codebook_ on y = project_in(z): k-means of the projected rows (of y^ with cosine_sim)."""
        _need_hip_f32(z, "init_codebook_")
        y = F_hip.linear_rows(z.detach(), self.project_in.weight.detach(), self.project_in.bias.detach(), rowmajor=rowmajor)
        return self._INNER.init_codebook_(self, y, iters, generator, rowmajor=rowmajor)


class FactorizedVectorQuantizerEMA(FactorizedVectorQuantizer, VectorQuantizerEMA):
    """FactorizedVectorQuantizer whose (n_e, codebook_dim) codebook follows exponential moving averages: VectorQuantizerEMA between
    the two projections.  State: FactorizedVectorQuantizer's, and the buffers `ema_cluster_size` (K,) and `ema_w` (K, codebook_dim).
    The update runs from y = project_in(z) (from y^ with cosine_sim) and that forward's indices, in training mode only, after the
    inner quantizer's outputs are formed; the projections are trained by their gradients.  With init_codebook_ the EMA state
    continues from the clusters, as VectorQuantizerEMA's does.  sync / accumulate: VectorQuantizerEMA's, the records taken from y
    (y^ with cosine_sim) exactly where the update reads."""

    _INNER = VectorQuantizerEMA

    def __init__(self, n_e, dim, codebook_dim, beta, decay=0.99, eps=1e-5, restart_threshold=None, generator=None, *,
                 rotation_trick=False, cosine_sim=False, entropy_weight=0.0, entropy_diversity_gamma=1.0,
                 entropy_inv_temperature=100.0, sync=False, accumulate=1):
        dim, codebook_dim = self._check_dims(dim, codebook_dim)
        VectorQuantizerEMA.__init__(self, n_e, codebook_dim, beta, decay, eps, restart_threshold, generator,
                                    rotation_trick=rotation_trick, cosine_sim=cosine_sim, entropy_weight=entropy_weight,
                                    entropy_diversity_gamma=entropy_diversity_gamma,
                                    entropy_inv_temperature=entropy_inv_temperature, sync=sync, accumulate=accumulate)
        self._init_projections(dim, codebook_dim)


class ResidualVectorQuantizer(nn.Module):
    """Residual quantization (RQ-VAE, arXiv 2203.01941; SoundStream's RVQ): n_q codebooks quantize the same latent position, each
    stage -- the reference's quantizer as written -- what the stage before it left over; z_q is z + (sum of the stages' codes - z)
    and the loss the sum of the stages' losses (csrc/vq_residual.hip states the arithmetic).

    Stage 0's codebook is `embedding` (VectorQuantizer's state_dict key: a reference checkpoint fills it); stages 1 .. n_q - 1 are
    `residual_embeddings.{q-1}`, absent with shared_codebook, where every stage uses `embedding`.  Every codebook starts as
    uniform(-1/K, 1/K), like the reference's."""

    LAZY_MIN_ENCODINGS = True

    def __init__(self, n_q, n_e, e_dim, beta, shared_codebook=False):
        super().__init__()
        if not 1 <= int(n_q) <= 16:
            raise ValueError("n_q must be in [1, 16]")
        self.n_q = int(n_q)
        self.n_e = n_e
        self.e_dim = e_dim
        self.beta = beta
        self.shared_codebook = bool(shared_codebook)
        self.embedding = nn.Embedding(self.n_e, self.e_dim)
        self.embedding.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)
        if not self.shared_codebook:
            self.residual_embeddings = nn.ModuleList(nn.Embedding(self.n_e, self.e_dim) for _ in range(self.n_q - 1))
            for emb in self.residual_embeddings:
                emb.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)

    def codebooks(self):
        """the distinct codebooks in stage order (one when shared)"""
        if self.shared_codebook:
            return [self.embedding.weight]
        return [self.embedding.weight] + [emb.weight for emb in self.residual_embeddings]

    def invalidate(self):
        """Forget the prepared codebook images (VectorQuantizer.invalidate: after a write through `.data`)."""
        for slot in _cache.side(self).get("ws", {}).values():
            slot[1] = None

    def _workspace(self, N):
        """-> (workspace, prepared, key, slot), one per (device, stream, N): VectorQuantizer._workspace with every stage's image"""
        ws_ = self.codebooks()
        w = ws_[0]
        key = tuple((t.data_ptr(), t._version) for t in ws_) + (w.device,)
        table = _cache.side(self).setdefault("ws", {})
        skey = (str(w.device), torch.cuda.current_stream(w.device).cuda_stream if w.is_cuda else 0, N)
        slot = _cache.lru_get(table, skey)
        if slot is None:
            slot = [F_hip.vq_residual_workspace(N, self.n_e, self.e_dim, self.n_q, w.device, shared=self.shared_codebook), None]
            _cache.lru_put(table, skey, slot, 8)
        return slot[0], slot[1] == key, key, slot

    def quantize(self, z, *, rowmajor=False, want_zq=True):
        """-> (loss, z_q, perplexity (n_q,), idx (n_q, N), hist (n_q, K)); no one-hot."""
        books = self.codebooks()
        N = z.numel() // self.e_dim
        ws, prepared, key, slot = self._workspace(N)
        if not prepared:
            slot[1] = None
        if torch.is_grad_enabled() and (z.requires_grad or any(w.requires_grad for w in books)):
            from .training import RVQStraightThrough           # HIP forward + HIP backward
            out = RVQStraightThrough.apply(z, self.beta, rowmajor, self.shared_codebook, self.n_q, ws, prepared, *books)
        else:
            out = F_hip.vq_residual_forward(z, [w.detach() for w in books], self.beta, rowmajor=rowmajor,
                                            shared=self.shared_codebook, n_q=self.n_q, workspace=ws, prepared=prepared,
                                            want_zq=want_zq)
        slot[1] = key
        return out[:5]

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    @torch.no_grad()
    def init_codebook_(self, z, iters=10, generator=None, *, rowmajor=False):
        """Opt-in data-dependent start, stage by stage: E_q = k-means (functional.vq_kmeans) of the rows of r_q, then one assignment
        against it and one advance r_{q+1} = r_q - E_q[idx_q], r_0 = z.  shared_codebook: k-means of z only.
        -> [(codebook, counts of the last assignment)] per distinct codebook."""
        _need_hip_f32(z, "init_codebook_")
        r = z.detach().contiguous()
        out = []
        books = self.codebooks()
        for q, w in enumerate(books):
            codebook, counts = F_hip.vq_kmeans(r, self.n_e, iters, generator=generator, rowmajor=rowmajor)
            w.copy_(codebook)
            out.append((codebook, counts))
            if q + 1 < len(books):
                r = F_hip.vq_residual_forward(r, [codebook], 0.0, rowmajor=rowmajor, want_zq=False, want_residual=True)[6]
        return out

    def forward(self, z, *, rowmajor=False):
        """The reference's 5-tuple shape: (loss, z_q, perplexity (n_q,), stage 0's min_encodings, idx (n_q, N)).  rowmajor: z and
        z_q are (B,H,W,D), as VQVAE.forward hands them over."""
        loss, z_q, perplexity, idx, _ = self.quantize(z, rowmajor=rowmajor)
        idx0 = idx[0].reshape(-1, 1)
        min_encodings = LazyOneHot(idx0, self.n_e) if self.LAZY_MIN_ENCODINGS else F_hip.vq_onehot(idx0, self.n_e)
        return loss, z_q, perplexity, min_encodings, idx


class GroupedVectorQuantizer(nn.Module):
    """Grouped (product) quantization (wav2vec 2.0's groups, arXiv 2006.11477; vector-quantize-pytorch's heads with
    separate_codebook_per_head): the e_dim channels of a latent row are cut into n_g groups of d = e_dim / n_g channels and every
    group is quantized -- by the reference's quantizer as written -- against its own (n_e, d) codebook.  A position carries n_g
    indices; z_q holds the groups' codes side by side (straight-through: z + (e - z)) and the loss is the mean of the groups'
    losses, which is the reference's loss formula on the whole rows (csrc/vq_grouped.hip states the arithmetic).

    Group 0's codebook is `embedding` (VectorQuantizer's state_dict key, of shape (n_e, d)); groups 1 .. n_g - 1 are
    `group_embeddings.{g-1}`.  Every codebook starts as uniform(-1/K, 1/K), drawn in group order."""

    LAZY_MIN_ENCODINGS = True

    def __init__(self, n_g, n_e, e_dim, beta):
        super().__init__()
        if not 1 <= int(n_g) <= 16:
            raise ValueError("n_g must be in [1, 16]")
        if int(e_dim) % int(n_g):
            raise ValueError(f"e_dim ({e_dim}) must be a multiple of the number of groups ({n_g})")
        self.n_g = int(n_g)
        self.n_e = n_e
        self.e_dim = int(e_dim)
        self.g_dim = self.e_dim // self.n_g
        self.beta = beta
        self.embedding = nn.Embedding(self.n_e, self.g_dim)
        self.embedding.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)
        self.group_embeddings = nn.ModuleList(nn.Embedding(self.n_e, self.g_dim) for _ in range(self.n_g - 1))
        for emb in self.group_embeddings:
            emb.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)

    def codebooks(self):
        """the codebooks in group order"""
        return [self.embedding.weight] + [emb.weight for emb in self.group_embeddings]

    def invalidate(self):
        """Forget the prepared codebook images (VectorQuantizer.invalidate: after a write through `.data`)."""
        for slot in _cache.side(self).get("ws", {}).values():
            slot[1] = None

    def _workspace(self, N):
        """-> (workspace, prepared, key, slot), one per (device, stream, N): VectorQuantizer._workspace with every group's image"""
        books = self.codebooks()
        w = books[0]
        key = tuple((t.data_ptr(), t._version) for t in books) + (w.device,)
        table = _cache.side(self).setdefault("ws", {})
        skey = (str(w.device), torch.cuda.current_stream(w.device).cuda_stream if w.is_cuda else 0, N)
        slot = _cache.lru_get(table, skey)
        if slot is None:
            slot = [F_hip.vq_grouped_workspace(N, self.n_e, self.e_dim, self.n_g, w.device), None]
            _cache.lru_put(table, skey, slot, 8)
        return slot[0], slot[1] == key, key, slot

    def _run(self, z, rowmajor, want_zq, *, commitment=False, want_slabs=False):
        """-> (loss, z_q, perplexity, idx, hist, loss_group, slabs or None) through the autograd pairing where a graph is recorded"""
        _need_hip_f32(z, type(self).__name__)
        books = self.codebooks()
        N = z.numel() // self.e_dim
        ws, prepared, key, slot = self._workspace(N)
        if not prepared:
            slot[1] = None
        if torch.is_grad_enabled() and (z.requires_grad or any(w.requires_grad for w in books)):
            from .training import GroupedStraightThrough       # HIP forward + HIP backward
            out = GroupedStraightThrough.apply(z, self.beta, rowmajor, commitment, want_slabs, ws, prepared, *books)
        else:
            out = F_hip.vq_grouped_forward(z, [w.detach() for w in books], 0.0 if commitment else self.beta, rowmajor=rowmajor,
                                           want_zq=want_zq, want_slabs=want_slabs, workspace=ws, prepared=prepared)
            if commitment:
                out = (out[0] * self.beta,) + out[1:5] + (out[5] * self.beta,) + out[6:]
            if not want_slabs:
                out = out + (None,)
        slot[1] = key
        return out

    def quantize(self, z, *, rowmajor=False, want_zq=True):
        """-> (loss, z_q, perplexity (n_g,), idx (n_g, N), hist (n_g, K)); no one-hot."""
        return self._run(z, rowmajor, want_zq)[:5]

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def _slabs(self, z, rowmajor):
        """the G dense slabs of z as the forward's split kernel writes them: (G,B,d,H,W), or (G,B,H,W,d) when rowmajor"""
        return F_hip.vq_grouped_forward(z.detach(), [w.detach() for w in self.codebooks()], 0.0, rowmajor=rowmajor, want_zq=False,
                                        want_slabs=True)[6]

    @torch.no_grad()
    def init_codebook_(self, z, iters=10, generator=None, *, rowmajor=False):
        """Opt-in data-dependent start, group by group: E_g = k-means (functional.vq_kmeans: k-means++ seeding and `iters` Lloyd
        rounds) of the group's slab of z.  -> [(codebook, counts of the last assignment)] in group order."""
        _need_hip_f32(z, "init_codebook_")
        out = []
        for w, slab in zip(self.codebooks(), self._slabs(z, rowmajor)):
            codebook, counts = F_hip.vq_kmeans(slab, self.n_e, iters, generator=generator, rowmajor=rowmajor)
            w.copy_(codebook)
            out.append((codebook, counts))
        return out

    def forward(self, z, *, rowmajor=False):
        """The reference's 5-tuple shape: (loss, z_q, perplexity (n_g,), group 0's min_encodings, idx (n_g, N)).  rowmajor: z and
        z_q are (B,H,W,D), as VQVAE.forward hands them over."""
        loss, z_q, perplexity, idx, _ = self.quantize(z, rowmajor=rowmajor)
        idx0 = idx[0].reshape(-1, 1)
        min_encodings = LazyOneHot(idx0, self.n_e) if self.LAZY_MIN_ENCODINGS else F_hip.vq_onehot(idx0, self.n_e)
        return loss, z_q, perplexity, min_encodings, idx


class GroupedVectorQuantizerEMA(_EMAMerge, GroupedVectorQuantizer):
    """GroupedVectorQuantizer whose codebooks follow exponential moving averages (VectorQuantizerEMA, per group) instead of a
    gradient.

    State: the codebooks (Parameters with requires_grad=False, GroupedVectorQuantizer's keys) and the buffers `ema_cluster_size`
    (n_g, K) = N_k per group (initially 0) and `ema_w` (n_g, K, d) = m_k (initially the initial codebooks).  Every forward in
    training mode -- with or without grad -- runs one update per group (vqvae_vq_ema_update_f32) from that forward's slab and
    indices, then copies the new codebooks in place.  Eval mode never updates.  The forward's outputs are those of the codebooks
    BEFORE the update; the loss is beta * the mean over the groups of the group's mse, and the codebooks get no gradient.

    restart_threshold: as VectorQuantizerEMA's, per group: one torch.rand(K) per group and update, drawn in group order.

    sync / accumulate: as VectorQuantizerEMA's (_EMAMerge): one record per group and training forward, one gather for all groups,
    one apply per group in group order; with restart one torch.rand(2, K) per group, in group order, at a cycle's first record."""

    def __init__(self, n_g, n_e, e_dim, beta, decay=0.99, eps=1e-5, restart_threshold=None, generator=None, *, sync=False,
                 accumulate=1):
        super().__init__(n_g, n_e, e_dim, beta)
        self.decay = float(decay)
        self.eps = float(eps)
        self.restart_threshold = None if restart_threshold is None else float(restart_threshold)
        self.generator = generator
        for w in self.codebooks():
            w.requires_grad_(False)
        self.register_buffer("ema_cluster_size", torch.zeros(self.n_g, n_e))
        self.register_buffer("ema_w", torch.stack([w.detach().clone() for w in self.codebooks()]))
        self._init_ema_merge(sync, accumulate)

    def invalidate(self):
        """GroupedVectorQuantizer.invalidate, and the pending statistics of an open sync / accumulate cycle are dropped."""
        super().invalidate()
        _cache.drop(self, "ema_pending")

    def _ema_states(self):
        return [(self.ema_cluster_size[g], self.ema_w[g], w) for g, w in enumerate(self.codebooks())]

    def _ema_update(self, slabs, idx, rowmajor):
        if self._ema_merging:
            return self._ema_record(list(slabs), list(idx), rowmajor)
        books = self.codebooks()
        dev = books[0].device
        N = idx.shape[1]
        wkey = (str(dev), torch.cuda.current_stream(dev).cuda_stream, N)
        table = _cache.side(self).setdefault("ema_ws", {})
        ws = _cache.lru_get(table, wkey)
        if ws is None:
            ws = F_hip.vq_ema_workspace(N, self.n_e, self.g_dim, dev)
            _cache.lru_put(table, wkey, ws, 4)
        for g, w in enumerate(books):
            uniforms = None
            if self.restart_threshold is not None:
                uniforms = torch.rand(self.n_e, device=dev, generator=self.generator)
            new = torch.empty_like(w, memory_format=torch.contiguous_format)
            F_hip.vq_ema_update(slabs[g], idx[g], self.ema_cluster_size[g], self.ema_w[g], new, self.decay, self.eps,
                                threshold=self.restart_threshold, uniforms=uniforms, rowmajor=rowmajor, workspace=ws)
            with torch.no_grad():
                w.copy_(new)

    @torch.no_grad()
    def init_codebook_(self, z, iters=10, generator=None, *, rowmajor=False):
        """GroupedVectorQuantizer.init_codebook_, and the EMA state continues from the clusters: ema_cluster_size[g] = counts,
        ema_w[g] = counts[:, None] * codebook."""
        out = super().init_codebook_(z, iters, generator, rowmajor=rowmajor)
        _cache.drop(self, "ema_pending")
        for g, (codebook, counts) in enumerate(out):
            c = counts.to(torch.float32)
            self.ema_cluster_size[g].copy_(c)
            self.ema_w[g].copy_(c[:, None] * codebook)
        return out

    def quantize(self, z, *, rowmajor=False, want_zq=True):
        """-> (beta * mean of the groups' mse, z_q, perplexity (n_g,), idx (n_g, N), hist (n_g, K)) against the codebooks as they
        were on entry; then, in training mode, one EMA update per group from the slabs the forward wrote."""
        out = self._run(z, rowmajor, want_zq, commitment=True, want_slabs=self.training)
        if self.training:
            self._ema_update(out[6], out[3], rowmajor)
        return out[:5]


class FiniteScalarQuantizer(nn.Module):
    """Finite scalar quantization (arXiv 2309.15505; vector-quantize-pytorch's FSQ): the quantizer without a learned codebook.  A
    latent row is projected to d = len(levels) channels (`project_in`), channel j is bounded with tanh and rounded to one of levels[j]
    values, and the codes are projected back (`project_out`); the implicit codebook has n_e = prod levels entries and every latent
    position still gets one integer index.  No commitment loss, no dead codes, no EMA state: the loss is a zero.  Both projections run
    inside the HIP kernels (csrc/vq_fsq.hip states the arithmetic); the state is the two nn.Linear layers and nothing else."""

    LAZY_MIN_ENCODINGS = True

    def __init__(self, levels, dim):
        super().__init__()
        self.levels, _, self.n_e = F_hip._fsq_levels(levels)
        if not 1 <= int(dim) <= 256:
            raise ValueError("dim must be in [1, 256]")
        self.e_dim = int(dim)
        self.project_in = nn.Linear(self.e_dim, len(self.levels))
        self.project_out = nn.Linear(len(self.levels), self.e_dim)

    def _params(self):
        return (self.project_in.weight, self.project_in.bias, self.project_out.weight, self.project_out.bias)

    def quantize(self, z, *, rowmajor=False, want_zq=True):
        """-> (zero loss, z_q, perplexity, indices (N,1), hist); no one-hot.  z: (B,D,H,W), or (B,H,W,D) when rowmajor."""
        _need_hip_f32(z, "FiniteScalarQuantizer")
        params = self._params()
        if torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for p in params)):
            from .training import FSQStraightThrough           # HIP forward + HIP backward
            z_q, perplexity, idx, hist = FSQStraightThrough.apply(z, *params, self.levels, rowmajor)
        else:
            z_q, perplexity, idx, hist = F_hip.fsq_forward(z, *[p.detach() for p in params], self.levels, rowmajor=rowmajor,
                                                           want_zq=want_zq)
        return torch.zeros((), dtype=torch.float32, device=z.device), z_q, perplexity, idx, hist

    def codes(self):
        """the (K, d) implicit codebook: row k holds the d codes q_j / (L_j // 2) of index k (first level least significant)"""
        dev = self.project_in.weight.device
        lv = torch.tensor(self.levels, dtype=torch.int64, device=dev)
        basis = torch.cumprod(torch.cat([lv.new_ones(1), lv[:-1]]), 0)
        hw = lv // 2
        q = (torch.arange(self.n_e, dtype=torch.int64, device=dev)[:, None] // basis[None, :]) % lv[None, :] - hw[None, :]
        return (q.to(torch.float64) / hw.to(torch.float64)[None, :]).to(torch.float32)

    @torch.no_grad()
    def codebook(self):
        """the (K, dim) decoded rows: what decode_indices writes for every index (functional.fsq_decode_indices)"""
        w, b = self.project_out.weight, self.project_out.bias
        _need_hip_f32(w, "FiniteScalarQuantizer.codebook")
        idx = torch.arange(self.n_e, dtype=torch.int64, device=w.device)
        return F_hip.fsq_decode_indices(idx, w.detach(), b.detach(), self.levels, self.n_e, 1, 1, rowmajor=True,
                                        validate=False).reshape(self.n_e, self.e_dim)

    def forward(self, z):
        loss, z_q, perplexity, idx, _ = self.quantize(z)
        min_encodings = LazyOneHot(idx, self.n_e) if self.LAZY_MIN_ENCODINGS else F_hip.vq_onehot(idx, self.n_e)
        return loss, z_q, perplexity, min_encodings, idx


class LookupFreeQuantizer(nn.Module):
    """Lookup-free quantization (MAGVIT-v2, arXiv 2310.05737 section 3.1; vector-quantize-pytorch's LFQ): the codebook is
    {-1, +1}^d with d = log2 n_e.  A latent row is projected to d channels (`project_in`), every channel keeps its sign, and the signs
    are projected back (`project_out`); every latent position still gets one integer index (first channel least significant).
    loss = beta * commitment + entropy_weight * (per-sample entropy - diversity_gamma * codebook entropy), computed by the HIP kernels
    from the factorised softmax (csrc/vq_lfq.hip states the arithmetic), in training and in eval mode.  The state is the two
    nn.Linear layers and nothing else."""

    LAZY_MIN_ENCODINGS = True

    def __init__(self, n_e, dim, beta, *, entropy_weight=0.1, diversity_gamma=1.0, inv_temperature=100.0):
        super().__init__()
        self.bits = F_hip._lfq_bits(n_e)
        if not 1 <= int(dim) <= 256:
            raise ValueError("dim must be in [1, 256]")
        self.n_e, self.e_dim, self.beta = int(n_e), int(dim), beta
        self.entropy_weight, self.diversity_gamma, self.inv_temperature = entropy_weight, diversity_gamma, inv_temperature
        self.project_in = nn.Linear(self.e_dim, self.bits)
        self.project_out = nn.Linear(self.bits, self.e_dim)
        self.last_losses = None                      # (loss, commitment, per-sample entropy, codebook entropy) of the latest call

    def _params(self):
        return (self.project_in.weight, self.project_in.bias, self.project_out.weight, self.project_out.bias)

    def _weights(self):
        return (float(self.beta), float(self.entropy_weight), float(self.diversity_gamma), float(self.inv_temperature))

    def quantize(self, z, *, rowmajor=False, want_zq=True, want_loss=True):
        """-> (loss (a zero without want_loss), z_q, perplexity, indices (N,1), hist); no one-hot.  z: (B,D,H,W), or (B,H,W,D) when
        rowmajor."""
        _need_hip_f32(z, "LookupFreeQuantizer")
        params = self._params()
        if want_loss and torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for p in params)):
            from .training import LFQStraightThrough           # HIP forward + HIP backward
            z_q, loss, perplexity, idx, hist, losses, _ = LFQStraightThrough.apply(z, *params, self.n_e, self._weights(), rowmajor)
        else:
            beta, we, gamma, inv_t = self._weights()
            z_q, perplexity, idx, hist, losses, _ = F_hip.lfq_forward(
                z, *[p.detach() for p in params], self.n_e, beta=beta, entropy_weight=we, diversity_gamma=gamma, inv_temperature=inv_t,
                rowmajor=rowmajor, want_zq=want_zq, want_loss=want_loss)
            loss = losses[0] if want_loss else torch.zeros((), dtype=torch.float32, device=z.device)
        if want_loss:
            self.last_losses = losses
        return loss, z_q, perplexity, idx, hist

    def codes(self):
        """the (K, d) implicit codebook: row k holds +1 where bit j of k is set, -1 where not (first channel least significant)"""
        dev = self.project_in.weight.device
        k = torch.arange(self.n_e, dtype=torch.int64, device=dev)[:, None]
        j = torch.arange(self.bits, dtype=torch.int64, device=dev)[None, :]
        return (((k >> j) & 1) * 2 - 1).to(torch.float32)

    def decode(self, idx, B, H, W, *, rowmajor=True, validate=True):
        """indices -> z_q rows (functional.lfq_decode_indices)"""
        return F_hip.lfq_decode_indices(idx.contiguous().view(-1).to(torch.int64), self.project_out.weight.detach(),
                                        self.project_out.bias.detach(), self.n_e, B, H, W, rowmajor=rowmajor, validate=validate)

    @torch.no_grad()
    def codebook(self):
        """the (K, dim) decoded rows: what decode_indices writes for every index"""
        w = self.project_out.weight
        _need_hip_f32(w, "LookupFreeQuantizer.codebook")
        idx = torch.arange(self.n_e, dtype=torch.int64, device=w.device)
        return self.decode(idx, self.n_e, 1, 1, validate=False).reshape(self.n_e, self.e_dim)

    def forward(self, z):
        loss, z_q, perplexity, idx, _ = self.quantize(z)
        min_encodings = LazyOneHot(idx, self.n_e) if self.LAZY_MIN_ENCODINGS else F_hip.vq_onehot(idx, self.n_e)
        return loss, z_q, perplexity, min_encodings, idx


class ResidualLayer(nn.Module):
    """Parameter holder mirroring models/residual.py:8-29."""

    def __init__(self, in_dim, h_dim, res_h_dim):
        super().__init__()
        self.res_block = nn.Sequential(
            nn.ReLU(True),
            nn.Conv2d(in_dim, res_h_dim, kernel_size=3, stride=1, padding=1, bias=False),
            nn.ReLU(True),
            nn.Conv2d(res_h_dim, h_dim, kernel_size=1, stride=1, bias=False),
        )

    def forward(self, x):
        return ResidualStack._run(x, [self], final_relu=False, mutate_input=True)


class ResidualStack(nn.Module):
    """n_res_layers aliases of ONE ResidualLayer (models/residual.py:41-51): the
    state_dict lists stack.0..n-1 keys that all share storage, exactly as upstream."""

    def __init__(self, in_dim, h_dim, res_h_dim, n_res_layers):
        super().__init__()
        self.n_res_layers = n_res_layers
        self.stack = nn.ModuleList([ResidualLayer(in_dim, h_dim, res_h_dim)] * n_res_layers)

    @staticmethod
    def _run(x, layers, final_relu, mutate_input):
        from . import conv as C_hip
        if _records_graph(x, *[p for l in layers for p in l.parameters()]):
            # under autograd the caller's tensor is NOT rewritten to relu(x) (upstream's in-place nn.ReLU does that through
            # autograd's version counter; an out-of-graph write here would corrupt other consumers' gradients): use the return value
            from . import autograd_conv as A_hip
            _need_hip_f32(x, "ResidualStack.forward")
            return A_hip.residual_stack_forward_train(x, layers, final_relu)
        y = C_hip.residual_stack_nchw(x, layers, final_relu=final_relu)
        if mutate_input:
            # nn.ReLU(True) upstream rewrites the caller's tensor to relu(x) (residual.py:19)
            x.relu_()
        return y

    def forward(self, x):
        return ResidualStack._run(x, list(self.stack), final_relu=True, mutate_input=True)


class Encoder(nn.Module):
    """q_theta(z|x) parameter holder mirroring models/encoder.py:24-43."""

    def __init__(self, in_dim, h_dim, n_res_layers, res_h_dim):
        super().__init__()
        kernel, stride = 4, 2
        self.conv_stack = nn.Sequential(
            nn.Conv2d(in_dim, h_dim // 2, kernel_size=kernel, stride=stride, padding=1),
            nn.ReLU(),
            nn.Conv2d(h_dim // 2, h_dim, kernel_size=kernel, stride=stride, padding=1),
            nn.ReLU(),
            nn.Conv2d(h_dim, h_dim, kernel_size=kernel - 1, stride=stride - 1, padding=1),
            ResidualStack(h_dim, h_dim, res_h_dim, n_res_layers),
        )

    def forward(self, x):
        from . import conv as C_hip
        if _records_graph(x, *self.parameters()):
            from . import autograd_conv as A_hip
            _need_hip_f32(x, "Encoder.forward")
            return A_hip.encoder_stack_forward_train(self, x)
        return C_hip.encoder_forward(self, x, pre_quant=None)


class Decoder(nn.Module):
    """p_phi(x|z) parameter holder mirroring models/decoder.py:22-39."""

    def __init__(self, in_dim, h_dim, n_res_layers, res_h_dim):
        super().__init__()
        kernel, stride = 4, 2
        self.inverse_conv_stack = nn.Sequential(
            nn.ConvTranspose2d(in_dim, h_dim, kernel_size=kernel - 1, stride=stride - 1, padding=1),
            ResidualStack(h_dim, h_dim, res_h_dim, n_res_layers),
            nn.ConvTranspose2d(h_dim, h_dim // 2, kernel_size=kernel, stride=stride, padding=1),
            nn.ReLU(),
            nn.ConvTranspose2d(h_dim // 2, 3, kernel_size=kernel, stride=stride, padding=1),
        )

    def forward(self, x):
        from . import conv as C_hip
        if _records_graph(x, *self.parameters()):
            from . import autograd_conv as A_hip
            _need_hip_f32(x, "Decoder.forward")
            return A_hip.decoder_forward_train(self, x.permute(0, 2, 3, 1).contiguous())
        return C_hip.decoder_forward(self, x, rowmajor_in=False)


def _invalidate_after_load(module, incompatible):
    """load_state_dict post-hook (a module-level function: a local lambda here made the model unpicklable)."""
    module.invalidate_caches()


class VQVAE(nn.Module):
    """Mirrors models/vqvae.py:10-44."""

    def __init__(self, h_dim, res_h_dim, n_res_layers, n_embeddings, embedding_dim, beta,
                 save_img_embedding_map=False, *, ema_decay=None, ema_eps=1e-5, restart_threshold=None, n_quantizers=1,
                 shared_codebook=False, rotation_trick=False, cosine_sim=False, fsq_levels=None, codebook_groups=1,
                 lookup_free=False, lfq_entropy_weight=0.1, lfq_diversity_gamma=1.0, lfq_inv_temperature=100.0,
                 orthogonal_reg_weight=0.0, orthogonal_reg_active_codes_only=False, orthogonal_reg_max_codes=None,
                 ema_sync=False, ema_accumulate=1, entropy_weight=0.0, entropy_diversity_gamma=1.0, entropy_inv_temperature=100.0,
                 codebook_dim=None):
        super().__init__()
        # ema_sync / ema_accumulate: the EMA quantizers' sync / accumulate (_EMAMerge): the codebook moves once per ema_accumulate
        # training forwards, from the statistics of those batches merged -- with ema_sync across the process group's ranks too
        ema_accumulate = _EMAMerge._check_accumulate(ema_accumulate)
        if ema_decay is None and (ema_sync or ema_accumulate != 1):
            raise ValueError("ema_sync / ema_accumulate need the EMA codebook (ema_decay)")
        merge = dict(sync=bool(ema_sync), accumulate=ema_accumulate)
        # entropy_weight > 0: the code-entropy loss of the learned codebook (csrc/vq_entropy.hip) joins the training loss of the
        # one-stage quantizers -- plain, EMA (only z takes its gradient), cosine_sim (on the unit rows: entropy_inv_temperature = 50
        # is MaskGIT's temperature of 0.01), rotation_trick, codebook_dim (on the projected rows)
        entropy_weight, entropy_diversity_gamma, entropy_inv_temperature = VectorQuantizer._check_entropy(
            entropy_weight, entropy_diversity_gamma, entropy_inv_temperature)
        if entropy_weight > 0.0:
            for name, on in (("n_quantizers > 1", n_quantizers != 1), ("shared_codebook", shared_codebook),
                             ("codebook_groups > 1", codebook_groups != 1), ("fsq_levels", fsq_levels is not None),
                             ("lookup_free (which has its own entropy loss: lfq_entropy_weight)", lookup_free)):
                if on:
                    raise ValueError(f"entropy_weight > 0 does not combine with {name}")
        ent = dict(entropy_weight=entropy_weight, entropy_diversity_gamma=entropy_diversity_gamma,
                   entropy_inv_temperature=entropy_inv_temperature)
        orthogonal_reg_weight, orthogonal_reg_max_codes = VectorQuantizer._check_orthogonal(orthogonal_reg_weight,
                                                                                           orthogonal_reg_max_codes)
        if orthogonal_reg_weight > 0.0:
            # the orthogonal regularization loss trains the codebook by its gradient: the one-stage gradient-trained quantizers
            for name, on in (("ema_decay (no gradient reaches an EMA codebook)", ema_decay is not None),
                             ("n_quantizers > 1", n_quantizers != 1), ("codebook_groups > 1", codebook_groups != 1),
                             ("fsq_levels", fsq_levels is not None), ("lookup_free", lookup_free)):
                if on:
                    raise ValueError(f"orthogonal_reg_weight > 0 does not combine with {name}")
        orth = dict(orthogonal_reg_weight=orthogonal_reg_weight, orthogonal_reg_active_codes_only=orthogonal_reg_active_codes_only,
                    orthogonal_reg_max_codes=orthogonal_reg_max_codes)
        if codebook_dim is not None:
            # factorized codes: the plain or the EMA quantizer between two projections, with the one-stage quantizers' options
            FactorizedVectorQuantizer._check_dims(embedding_dim, codebook_dim)
            for name, on in (("n_quantizers > 1", n_quantizers != 1), ("shared_codebook", shared_codebook),
                             ("codebook_groups > 1", codebook_groups != 1), ("fsq_levels", fsq_levels is not None),
                             ("lookup_free", lookup_free)):
                if on:
                    raise ValueError(f"codebook_dim (factorized codes) does not combine with {name}")
        if lookup_free:
            # lookup-free quantization: the codebook is {-1, +1}^d; beta weighs its commitment term
            for name, on in (("ema_decay", ema_decay is not None), ("restart_threshold", restart_threshold is not None),
                             ("n_quantizers > 1", n_quantizers != 1), ("shared_codebook", shared_codebook),
                             ("rotation_trick", rotation_trick), ("cosine_sim", cosine_sim), ("fsq_levels", fsq_levels is not None),
                             ("codebook_groups > 1", codebook_groups != 1)):
                if on:
                    raise ValueError(f"lookup_free (lookup-free quantization) has no learned codebook: {name} does not apply")
            F_hip._lfq_bits(n_embeddings)
        if codebook_groups != 1:
            # grouped (product) quantization: every group is the plain or the EMA quantizer on its channels, nothing else
            if not 1 <= int(codebook_groups) <= 16:
                raise ValueError("codebook_groups must be in [1, 16]")
            for name, on in (("n_quantizers > 1", n_quantizers != 1), ("shared_codebook", shared_codebook),
                             ("rotation_trick", rotation_trick), ("cosine_sim", cosine_sim), ("fsq_levels", fsq_levels is not None)):
                if on:
                    raise ValueError(f"codebook_groups > 1 (grouped quantization) does not combine with {name}")
            if embedding_dim % int(codebook_groups):
                raise ValueError(f"embedding_dim ({embedding_dim}) must be a multiple of codebook_groups ({codebook_groups})")
        if fsq_levels is not None:
            # finite scalar quantization has no codebook: nothing that trains, restarts, stacks, rotates towards or normalises one
            for name, on in (("ema_decay", ema_decay is not None), ("restart_threshold", restart_threshold is not None),
                             ("n_quantizers > 1", n_quantizers != 1), ("shared_codebook", shared_codebook),
                             ("rotation_trick", rotation_trick), ("cosine_sim", cosine_sim)):
                if on:
                    raise ValueError(f"fsq_levels (finite scalar quantization) has no learned codebook: {name} does not apply")
            fsq_levels, _, k = F_hip._fsq_levels(fsq_levels)
            if k != n_embeddings:
                raise ValueError(f"n_embeddings must be the product of fsq_levels ({k}), got {n_embeddings}")
        if n_quantizers > 1 and cosine_sim:
            raise ValueError("cosine_sim is the one-stage quantizers' option: a per-stage normalisation of residual quantization "
                             "(n_quantizers > 1) does not exist")
        if n_quantizers > 1 and rotation_trick:
            raise ValueError("rotation_trick is the one-stage quantizers' option: residual quantization (n_quantizers > 1) has none")
        if n_quantizers < 1:
            raise ValueError("n_quantizers must be >= 1")
        if n_quantizers > 1 and ema_decay is not None:
            raise ValueError("residual quantization (n_quantizers > 1) has no EMA codebook update: leave ema_decay unset")
        if n_quantizers == 1 and shared_codebook:
            raise ValueError("shared_codebook needs n_quantizers > 1")
        self.encoder = Encoder(3, h_dim, n_res_layers, res_h_dim)
        self.pre_quantization_conv = nn.Conv2d(h_dim, embedding_dim, kernel_size=1, stride=1)
        if codebook_groups != 1:
            if ema_decay is None:
                if restart_threshold is not None:
                    raise ValueError("restart_threshold needs the EMA codebook (ema_decay)")
                self.vector_quantization = GroupedVectorQuantizer(codebook_groups, n_embeddings, embedding_dim, beta)
            else:
                self.vector_quantization = GroupedVectorQuantizerEMA(codebook_groups, n_embeddings, embedding_dim, beta,
                                                                     decay=ema_decay, eps=ema_eps,
                                                                     restart_threshold=restart_threshold, **merge)
        elif fsq_levels is not None:
            self.vector_quantization = FiniteScalarQuantizer(fsq_levels, embedding_dim)       # (beta: accepted, unused)
        elif lookup_free:
            self.vector_quantization = LookupFreeQuantizer(n_embeddings, embedding_dim, beta, entropy_weight=lfq_entropy_weight,
                                                           diversity_gamma=lfq_diversity_gamma, inv_temperature=lfq_inv_temperature)
        elif n_quantizers > 1:
            if restart_threshold is not None:
                raise ValueError("restart_threshold needs the EMA codebook (ema_decay)")
            self.vector_quantization = ResidualVectorQuantizer(n_quantizers, n_embeddings, embedding_dim, beta,
                                                               shared_codebook=shared_codebook)
        elif codebook_dim is not None:
            if ema_decay is None:
                if restart_threshold is not None:
                    raise ValueError("restart_threshold needs the EMA codebook (ema_decay)")
                self.vector_quantization = FactorizedVectorQuantizer(n_embeddings, embedding_dim, codebook_dim, beta,
                                                                     rotation_trick=rotation_trick, cosine_sim=cosine_sim, **orth,
                                                                     **ent)
            else:
                self.vector_quantization = FactorizedVectorQuantizerEMA(n_embeddings, embedding_dim, codebook_dim, beta,
                                                                        decay=ema_decay, eps=ema_eps,
                                                                        restart_threshold=restart_threshold,
                                                                        rotation_trick=rotation_trick, cosine_sim=cosine_sim,
                                                                        **ent, **merge)
        elif ema_decay is None:
            if restart_threshold is not None:
                raise ValueError("restart_threshold needs the EMA codebook (ema_decay)")
            self.vector_quantization = VectorQuantizer(n_embeddings, embedding_dim, beta, rotation_trick=rotation_trick,
                                                       cosine_sim=cosine_sim, **orth, **ent)
        else:
            # the codebook by exponential moving averages (VectorQuantizerEMA); the random initialisation is VectorQuantizer's
            self.vector_quantization = VectorQuantizerEMA(n_embeddings, embedding_dim, beta, decay=ema_decay, eps=ema_eps,
                                                          restart_threshold=restart_threshold, rotation_trick=rotation_trick,
                                                          cosine_sim=cosine_sim, **ent, **merge)
        self.decoder = Decoder(embedding_dim, h_dim, n_res_layers, res_h_dim)
        if save_img_embedding_map:
            self.img_to_embedding_map = {i: [] for i in range(n_embeddings)}
        else:
            self.img_to_embedding_map = None
        self.register_load_state_dict_post_hook(_invalidate_after_load)

    def invalidate_caches(self):
        """Drop the prepared codebook image and every packed-weight image (they are keyed on the parameters'
        data_ptr / _version, which writes through `.data` do not change; `load_state_dict` calls this)."""
        from . import conv_hip
        _cache.drop(self, "c_weights")
        for mod in self.modules():
            conv_hip.invalidate(mod)
            if isinstance(mod, (VectorQuantizer, ResidualVectorQuantizer, GroupedVectorQuantizer)):
                mod.invalidate()

    # forward / encode / decode_indices follow vqvae_weights_range_check_f32's recommendation for the checkpoint (scheme_hint()) unless
    # the caller names a scheme.  False: never check (no host sync per weight version -- an eval forward after every optimizer step
    # pays one otherwise), always the default two-term fp16 products unless a scheme is named.
    AUTO_SCHEME = True

    # ---- whole-path C ABI (include/vqvae_hip.h: vqvae_forward_f32) ------------------------------------------------
    _RAW = {"enc0_w": "encoder.conv_stack.0.weight", "enc0_b": "encoder.conv_stack.0.bias",
            "enc2_w": "encoder.conv_stack.2.weight", "enc2_b": "encoder.conv_stack.2.bias",
            "enc4_w": "encoder.conv_stack.4.weight", "enc4_b": "encoder.conv_stack.4.bias",
            "enc_res_w1": "encoder.conv_stack.5.stack.0.res_block.1.weight",
            "enc_res_w2": "encoder.conv_stack.5.stack.0.res_block.3.weight",
            "pre_w": "pre_quantization_conv.weight", "pre_b": "pre_quantization_conv.bias",
            "codebook": "vector_quantization.embedding.weight",
            "dec0_w": "decoder.inverse_conv_stack.0.weight", "dec0_b": "decoder.inverse_conv_stack.0.bias",
            "dec_res_w1": "decoder.inverse_conv_stack.1.stack.0.res_block.1.weight",
            "dec_res_w2": "decoder.inverse_conv_stack.1.stack.0.res_block.3.weight",
            "dec2_w": "decoder.inverse_conv_stack.2.weight", "dec2_b": "decoder.inverse_conv_stack.2.bias",
            "dec4_w": "decoder.inverse_conv_stack.4.weight", "dec4_b": "decoder.inverse_conv_stack.4.bias"}

    def _c_weights(self):
        """-> (VqvaeWeights, keep-alive tensors): every layer packed once per weight version into ONE buffer by
        vqvae_weights_pack_f32; rebuilt when any parameter's (data_ptr, _version) or the quantizer's beta changes, or invalidate_caches() ran."""
        from . import _lib
        if isinstance(self.vector_quantization, FiniteScalarQuantizer):
            raise VqvaeHipError("the fused whole-path entries have no finite scalar quantizer: FSQ models run layer by layer")
        if isinstance(self.vector_quantization, LookupFreeQuantizer):
            raise VqvaeHipError("the fused whole-path entries have no lookup-free quantizer: LFQ models run layer by layer")
        if isinstance(self.vector_quantization, GroupedVectorQuantizer):
            raise VqvaeHipError("the fused whole-path entries quantize whole rows: grouped models run layer by layer")
        if isinstance(self.vector_quantization, FactorizedVectorQuantizer):
            raise VqvaeHipError("the fused whole-path entries search a codebook of embedding_dim channels: factorized models "
                                "(codebook_dim) run layer by layer")
        params = dict(self.named_parameters(remove_duplicate=False))
        n_res = self.encoder.conv_stack[5].n_res_layers
        tensors = {}
        for f, k in self._RAW.items():
            if k not in params:                       # n_res_layers == 0: no residual weights; the stack is skipped
                tensors[f] = params["encoder.conv_stack.4.weight"]
            else:
                tensors[f] = params[k]
        # beta is packed into VqvaeDims: a changed m.vector_quantization.beta must repack, as models/quantizer.py:63-64 reads it per call
        key = tuple((t.data_ptr(), t._version) for t in tensors.values()) + (str(tensors["enc0_w"].device),
                                                                              self._packed_beta())
        hit = _cache.side(self).get("c_weights")
        if hit is not None and hit[0] == key:
            _cache.wait_ready(hit[3], tensors["enc0_w"].device)          # packed on another stream a moment ago?
            return hit[1], hit[2]
        L = _lib.load()
        w0 = tensors["enc0_w"]
        dims = _lib.VqvaeDims(self.encoder.conv_stack[4].weight.shape[0], tensors["enc_res_w1"].shape[0] if n_res else 1,
                              n_res, self.vector_quantization.n_e, self.vector_quantization.e_dim, w0.shape[1],
                              self._packed_beta())
        nbytes = L.vqvae_weights_packed_bytes(dims)
        if nbytes == 0:
            raise VqvaeHipError("model dimensions not supported by the gfx950 whole-path entry points")
        keep = {f: _lib.dense(t.detach()) for f, t in tensors.items()}
        raw = _lib.VqvaeRawWeights(**{f: t.data_ptr() for f, t in keep.items()})
        packed = torch.empty(nbytes, dtype=torch.uint8, device=w0.device)
        cw = _lib.VqvaeWeights()
        with torch.cuda.device(w0.device):
            _lib.check(L.vqvae_weights_pack_f32(dims, raw, packed.data_ptr(), nbytes, cw,
                                                torch.cuda.current_stream(w0.device).cuda_stream))
            # which product scheme this checkpoint calls for (vqvae_weights_range_check_f32: once per weight version, one sync).
            # Not while a stream capture is recording (the check synchronises): the previous version's hint stands, or none.
            import ctypes
            rec = ctypes.c_int(0)
            spreads = (ctypes.c_float * 11)()
            hint = None
            if self.AUTO_SCHEME and not torch.cuda.is_current_stream_capturing():
                scratch = torch.empty(16, dtype=torch.float32, device=w0.device)
                _lib.check(L.vqvae_weights_range_check_f32(dims, raw, spreads, ctypes.byref(rec), scratch.data_ptr(), 64,
                                                           torch.cuda.current_stream(w0.device).cuda_stream))
                hint = (int(rec.value), [float(v) for v in spreads])
            elif self.AUTO_SCHEME:
                hint = _cache.side(self).get("c_scheme_hint")
                import warnings
                warnings.warn("VQVAE: new weights met inside a stream capture -- the range check (a host sync) is skipped and "
                              + ("the previous weights' product scheme is kept" if hint else "the default two-term fp16 scheme is used")
                              + "; run one forward outside the capture first, or name a scheme (fwd_flags)", RuntimeWarning, stacklevel=3)
            ready = _cache.mark_ready(w0.device)
        if hint is None:
            hint = (0, [0.0] * 11)
        old = _cache.side(self).get("c_scheme_hint")
        if hint[0] and (old is None or old[0] != hint[0]):
            # the whole path changes kernels, numerics and speed with this: say so once per flip, never silently
            import warnings
            warnings.warn(f"VQVAE: this checkpoint's weights spread over {max(hint[1]):.1f} binades of input-channel magnitude in one layer "
                          "(limit 10): forward / encode / decode_indices run the three-term bf16 scheme (VQVAE_FWD_CONV_BF16_SPLIT, about "
                          "half the speed of the default two-term fp16 products).  Name a scheme (fwd_flags=...) or set "
                          "VQVAE.AUTO_SCHEME = False to decide yourself", RuntimeWarning, stacklevel=3)
        _cache.side(self)["c_weights"] = (key, cw, (keep, packed), ready)
        _cache.side(self)["c_scheme_hint"] = hint
        return cw, (keep, packed)

    def _packed_beta(self):
        """beta as the whole path's loss reads it: the reference's (1 + beta) mse for VectorQuantizer; for VectorQuantizerEMA 0, so
        that the path returns mse itself and forward() scales it to the commitment loss beta * mse"""
        return 0.0 if isinstance(self.vector_quantization, VectorQuantizerEMA) else float(self.vector_quantization.beta)

    def scheme_hint(self):
        """-> (flags, per-layer input-channel spread in binades): FWD_CONV_BF16_SPLIT when this checkpoint's weights put the default
        two-term fp16 products outside their range (include/vqvae_hip.h, vqvae_weights_range_check_f32), else 0.  forward / encode /
        decode_indices apply it unless the caller names a scheme."""
        self._c_weights()
        return _cache.side(self)["c_scheme_hint"]

    # The step can run as n parts on n side streams (vqvae_forward_begin / part / end; _forward_c(x, parts=n)): the kernels of
    # different parts fill each other's ramp-up and tail.  NOT the default: measured -2 % per step on one MI355X box and +9 % on
    # another (profiles/r03_notes.txt section 11), so FORWARD_PARTS stays 1 = one vqvae_forward_f32 call on the current stream.
    FORWARD_PARTS = 1
    FORWARD_PARTS_MIN_BATCH = 2048

    def _forward_parts(self, L, cw, x, B, H, W, flags, x_hat, scal, idx, ws, nws, vws, dev, stream, parts):
        """The step in parts on side streams; False = not applicable here (the caller makes the single call).  Outputs are
        bit-identical to the single call; the current stream waits for the side streams before this returns."""
        from . import _lib
        n = self.FORWARD_PARTS if parts is None else parts
        if n < 2 or B < (self.FORWARD_PARTS_MIN_BATCH if parts is None else 128) or (H, W) != (32, 32):
            return False
        rc = L.vqvae_forward_begin_f32(cw, B, H, W, flags, ws.data_ptr(), nws, vws.data_ptr(), vws.numel(), stream)
        if rc == -3:                                   # VQVAE_ERR_UNSUPPORTED: another architecture / codebook shape / quantizer flags
            return False
        _lib.check(rc)
        pool = _cache.side(self).setdefault("part_streams", {})
        streams = pool.get(str(dev))
        if streams is None or len(streams) < n:
            streams = pool[str(dev)] = [torch.cuda.Stream(device=dev) for _ in range(n)]
        cur = torch.cuda.current_stream(dev)
        per = -(-B // n)
        per = -(-per // 64) * 64                        # whole 64-image blocks per part
        b0 = 0
        used = []
        try:
            for s in streams[:n]:
                if b0 >= B:
                    break
                bc = min(per, B - b0)
                s.wait_stream(cur)
                used.append(s)                                  # (before the launch: a failing part may have enqueued kernels already)
                _lib.check(L.vqvae_forward_part_f32(cw, x.data_ptr(), B, b0, bc, H, W, flags, x_hat.data_ptr(),
                                                    idx.data_ptr() if idx is not None else None, ws.data_ptr(), nws, vws.data_ptr(),
                                                    vws.numel(), s.cuda_stream))
                b0 += bc
        except BaseException:
            L.vqvae_forward_abort_f32(ws.data_ptr())              # the step will not be finished: drop its host-side record
            raise
        finally:
            # ALWAYS: the caller's stream must not free or reuse x_hat / ws / idx while a side stream still writes them, also
            # when a part raised
            for s in used:
                cur.wait_stream(s)
        _lib.check(L.vqvae_forward_end_f32(cw, B, H, W, scal.data_ptr(), scal.data_ptr() + 4, ws.data_ptr(), nws, stream))
        return True

    def _forward_c(self, x, want_idx=False, vq_flags=0, parts=None, fwd_flags=None):
        """VQVAE.forward as ONE call into libvqvae_hip.so (vqvae_forward_f32).  vq_flags: extra quantizer flags for tests and
        A/B runs (functional.VQ_UNFUSED: the quantizer as its own launch where the encoder's last kernel would quantize).
        parts: None = the default policy (FORWARD_PARTS side streams for large batches), 1 = always the single call, n = n parts.
        fwd_flags: functional.FWD_CONV_BF16_SPLIT / FWD_CONV_EXACT_FP32 = the whole path on the three-term bf16 / exact-fp32 MFMA
        kernels instead of the default two-term fp16 products; 0 = the two-term fp16 products whatever the weights; None (default) =
        what vqvae_weights_range_check_f32 recommends for this checkpoint (scheme_hint())."""
        from . import _lib
        L = _lib.load()
        x = _lib.dense(x)
        B, Cin, H, W = x.shape
        cw, _keep = self._c_weights()
        if fwd_flags is None:
            fwd_flags = _cache.side(self)["c_scheme_hint"][0]
        if Cin != cw.dims.in_ch or H % 4 or W % 4:
            raise ValueError(f"expected (B, {cw.dims.in_ch}, 4k, 4m) images, got {tuple(x.shape)}")
        dev = x.device
        with torch.cuda.device(dev):
            nws = L.vqvae_workspace_bytes(cw.dims, B, H, W)
            if nws == 0:
                raise VqvaeHipError(f"shape {tuple(x.shape)} not supported by the gfx950 whole-path entry points")
            # one activation workspace per (shape, device, stream), reused: forwards on different streams never share one
            stream = torch.cuda.current_stream(dev).cuda_stream
            # (keyed on (device, stream) only: ONE buffer per stream, grown to the largest batch seen -- a model that alternates
            # a training and an evaluation batch size keeps one workspace, not one per size)
            wkey = (str(dev), stream)
            table = _cache.side(self).setdefault("c_ws", {})
            ws = _cache.lru_get(table, wkey)
            if ws is None or ws.numel() < nws:
                ws = torch.empty(nws, dtype=torch.uint8, device=dev)
                _cache.lru_put(table, wkey, ws, 4)
            nws = ws.numel()
            vq = self.vector_quantization
            vws, prepared, key, slot = vq._workspace()
            if not prepared:
                slot[1] = None
            x_hat = torch.empty_like(x)
            scal = torch.empty(2, dtype=torch.float32, device=dev)
            idx = torch.empty((B * (H // 4) * (W // 4), 1), dtype=torch.int64, device=dev) if want_idx else None
            flags = (F_hip.VQ_CODEBOOK_PREPARED if prepared else 0) | vq_flags | fwd_flags
            if not self._forward_parts(L, cw, x, B, H, W, flags, x_hat, scal, idx, ws, nws, vws, dev, stream, parts):
                _lib.check(L.vqvae_forward_f32(cw, x.data_ptr(), B, H, W, flags, x_hat.data_ptr(), scal.data_ptr(), scal.data_ptr() + 4,
                                               idx.data_ptr() if want_idx else None, ws.data_ptr(), nws, vws.data_ptr(), vws.numel(),
                                               stream))
            slot[1] = key
        return (scal[0], x_hat, scal[1]) + ((idx,) if want_idx else ())

    def forward(self, x, verbose=False):
        from . import conv as C_hip
        if (C_hip.get_conv_backend() == "hip" and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters())):
            # training (main.py:74-79): every layer forward AND backward on the HIP kernels
            from . import autograd_conv as A_hip
            if not x.is_cuda or x.dtype != torch.float32:
                raise VqvaeHipError("VQVAE.forward needs a CUDA(HIP) fp32 input: there is no CPU path")
            z_e = A_hip.encoder_forward_train(self.encoder, x, self.pre_quantization_conv)
            if isinstance(self.vector_quantization, (ResidualVectorQuantizer, GroupedVectorQuantizer)):
                # (through the module's __call__: forward hooks see z_e; the stages' or groups' mean perplexity is the scalar
                # main.py:82 logs)
                embedding_loss, z_q, perplexity, _, _ = self.vector_quantization(z_e, rowmajor=True)
                perplexity = perplexity.mean()
            else:
                embedding_loss, z_q, perplexity, _, _ = self.vector_quantization.quantize(z_e, rowmajor=True)
            x_hat = A_hip.decoder_forward_train(self.decoder, z_q)
            return embedding_loss, x_hat, perplexity
        _require_forward_only(x, *self.parameters())
        vq = self.vector_quantization
        if isinstance(vq, ResidualVectorQuantizer):
            # residual stages: the per-layer path (the fused whole-path entries quantize once)
            if C_hip.get_conv_backend() == "hip":
                _need_hip_f32(x, "VQVAE.forward")
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            embedding_loss, z_q, perplexity, _, _ = vq(z_e, rowmajor=True)
            return embedding_loss, C_hip.decoder_forward(self.decoder, z_q, rowmajor_in=True), perplexity.mean()
        if isinstance(vq, GroupedVectorQuantizer):
            # groups: the per-layer path too.  Without a graph the decoder takes the code rows themselves, through the helper
            # decode_indices uses: decode_indices(encode(x)) is this x_hat bit for bit.  (The training forward decodes z + (e - z).)
            _need_hip_f32(x, "VQVAE.forward")
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            embedding_loss, _, perplexity, idx, _ = vq.quantize(z_e, rowmajor=True, want_zq=False)
            return embedding_loss, self._decode_grouped(idx, z_e.shape[0], z_e.shape[1], z_e.shape[2]), perplexity.mean()
        if isinstance(vq, (FiniteScalarQuantizer, LookupFreeQuantizer)):
            # the per-layer path too (an LFQ model's loss is computed here as well, as in training); the indices are decoded by the helper decode_indices uses: decode_indices(encode(x)) is this
            # x_hat bit for bit
            _need_hip_f32(x, "VQVAE.forward")
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            embedding_loss, _, perplexity, idx, _ = vq.quantize(z_e, rowmajor=True, want_zq=False)
            return embedding_loss, self._decode_fsq(idx, z_e.shape[0], z_e.shape[1], z_e.shape[2], validate=False), perplexity
        if isinstance(vq, FactorizedVectorQuantizer):
            # factorized codes: the per-layer path too (the fused entries must never see a (K, codebook_dim) codebook).  The decoder
            # takes rows of the decoded codebook through the helper decode_indices uses: decode_indices(encode(x)) is this x_hat
            # bit for bit -- the map is per row, so project_out(E[idx]) and project_out(E)[idx] have the same bits.  (The training
            # forward decodes project_out(y + (e - y)).)
            _need_hip_f32(x, "VQVAE.forward")
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            # (an EMA quantizer in training mode moves the codebook inside quantize: every output is the codebook's BEFORE the
            # update, so the decoded codebook is taken first)
            before = vq.codebook() if isinstance(vq, VectorQuantizerEMA) and vq.training else None
            embedding_loss, _, perplexity, idx, _ = vq.quantize(z_e, rowmajor=True, want_zq=False)
            return embedding_loss, self._decode_factorized(idx, z_e.shape[0], z_e.shape[1], z_e.shape[2], validate=False,
                                                           codebook=before), perplexity
        ema = isinstance(vq, VectorQuantizerEMA)
        # (an EMA quantizer in training mode updates its codebook from z_e: the per-layer path below materialises it; so does a
        # cosine_sim quantizer, whose rows are normalised between the encoder and the search -- the fused whole-path entries
        # quantize z_e as it stands)
        if (C_hip.get_conv_backend() == "hip" and not verbose and x.is_cuda and x.dtype == torch.float32
                and not (ema and vq.training) and not vq.cosine_sim):
            if ema:
                mse, x_hat, perplexity = self._forward_c(x)
                return mse * vq.beta, x_hat, perplexity
            return self._forward_c(x)                 # one ctypes call: vqvae_forward_f32
        # encoder + 1x1 pre-quantisation conv, activations kept row-major (B,H,W,C)
        z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
        if vq.cosine_sim and not verbose:
            # Without a graph nothing needs the straight-through form z^ + (e^ - z^), whose value is the code e^ up to one rounding:
            # the decoder takes the rows of E^ themselves, exactly as decode_indices does, so decode_indices(encode(x)) is this
            # x_hat bit for bit.  (The training forward decodes z^ + (e^ - z^): the gradient needs it.)
            embedding_loss, _, perplexity, idx, _ = vq.quantize(z_e, rowmajor=True, want_zq=False)
            return embedding_loss, self._decode_codes(idx, z_e.shape[0], z_e.shape[1], z_e.shape[2], validate=False), perplexity
        embedding_loss, z_q, perplexity, _, _ = self.vector_quantization.quantize(z_e, rowmajor=True)
        x_hat = C_hip.decoder_forward(self.decoder, z_q, rowmajor_in=True)
        if verbose:                                                    # models/vqvae.py:38-42
            print('original data shape:', x.shape)
            print('encoded data shape:', torch.Size((z_e.shape[0], z_e.shape[3], z_e.shape[1], z_e.shape[2])))
            print('recon data shape:', x_hat.shape)
            assert False
        return embedding_loss, x_hat, perplexity

    @torch.no_grad()
    def init_codebook_(self, x, iters=10, generator=None):
        """Opt-in: start the codebook on the data -- z_e of the images x from the encoder and pre_quantization_conv (HIP path, no
        grad), then the quantizer's init_codebook_ (k-means++ seeding and `iters` Lloyd rounds).  Call it before the first update."""
        from . import conv as C_hip
        if isinstance(self.vector_quantization, FiniteScalarQuantizer):
            raise VqvaeHipError("finite scalar quantization has no codebook to initialise")
        if isinstance(self.vector_quantization, LookupFreeQuantizer):
            raise VqvaeHipError("lookup-free quantization has no codebook to initialise")
        _need_hip_f32(x, "VQVAE.init_codebook_")
        if C_hip.get_conv_backend() != "hip":
            raise VqvaeHipError("VQVAE.init_codebook_ runs on the HIP conv backend: there is no fallback")
        z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)        # row-major (B,H,W,D)
        return self.vector_quantization.init_codebook_(z_e, iters, generator, rowmajor=True)

    # ---- "next" rows of SURVEY.md 8f-1: the index wire format -------------------
    def _c_workspace(self, L, cw, B, H, W, dev):
        """(workspace tensor, stream handle) of the whole-path C entry points for this device's current stream (see _forward_c)."""
        nws = L.vqvae_workspace_bytes(cw.dims, B, H, W)
        if nws == 0:
            raise VqvaeHipError(f"shape ({B}, {cw.dims.in_ch}, {H}, {W}) not supported by the gfx950 whole-path entry points")
        stream = torch.cuda.current_stream(dev).cuda_stream
        table = _cache.side(self).setdefault("c_ws", {})
        ws = _cache.lru_get(table, (str(dev), stream))
        if ws is None or ws.numel() < nws:
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            _cache.lru_put(table, (str(dev), stream), ws, 4)
        return ws, stream

    @torch.no_grad()
    def encode(self, x, vq_flags=0):
        """x -> min_encoding_indices (N,1) int64 (README.md:56; notebook encode_data) as ONE call into libvqvae_hip.so
        (vqvae_encode_f32): on the default shapes the encoder's last kernel quantizes its own z_e and only the indices are
        written -- no z_e, no z_q."""
        from . import _lib, conv as C_hip
        if isinstance(self.vector_quantization, ResidualVectorQuantizer):
            # (n_quantizers, N) int64, stage-major: the per-layer encoder, then the residual stages (indices only)
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            return self.vector_quantization.quantize(z_e, rowmajor=True, want_zq=False)[3]
        if isinstance(self.vector_quantization, GroupedVectorQuantizer):
            # (codebook_groups, N) int64, group-major; never an EMA update (GroupedVectorQuantizer's own quantize)
            _need_hip_f32(x, "VQVAE.encode")
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            return GroupedVectorQuantizer.quantize(self.vector_quantization, z_e, rowmajor=True, want_zq=False)[3]
        if isinstance(self.vector_quantization, FiniteScalarQuantizer):
            _need_hip_f32(x, "VQVAE.encode")
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            return self.vector_quantization.quantize(z_e, rowmajor=True, want_zq=False)[3]
        if isinstance(self.vector_quantization, LookupFreeQuantizer):
            _need_hip_f32(x, "VQVAE.encode")
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            return self.vector_quantization.quantize(z_e, rowmajor=True, want_zq=False, want_loss=False)[3]
        if isinstance(self.vector_quantization, FactorizedVectorQuantizer):
            # encoder -> linear_rows -> (l2norm_rows) -> index-only quantizer (VectorQuantizer's quantize: never an EMA update)
            _need_hip_f32(x, "VQVAE.encode")
            vq = self.vector_quantization
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            y = F_hip.linear_rows(z_e, vq.project_in.weight.detach(), vq.project_in.bias.detach(), rowmajor=True)
            return VectorQuantizer.quantize(vq, y, rowmajor=True, want_zq=False)[3]
        if (C_hip.get_conv_backend() != "hip" or not x.is_cuda or x.dtype != torch.float32
                or self.vector_quantization.cosine_sim):
            # (cosine_sim: encoder -> l2norm_rows -> index-only quantizer, the training forward's indices bit for bit)
            if self.vector_quantization.cosine_sim and C_hip.get_conv_backend() == "hip":
                _need_hip_f32(x, "VQVAE.encode")
            z_e = C_hip.encoder_forward(self.encoder, x, pre_quant=self.pre_quantization_conv)
            # (VectorQuantizer's quantize: an EMA quantizer in training mode must not update from encode())
            _, _, _, idx, _ = VectorQuantizer.quantize(self.vector_quantization, z_e, rowmajor=True, want_zq=False)
            return idx
        L = _lib.load()
        x = _lib.dense(x)
        B, Cin, H, W = x.shape
        cw, _keep = self._c_weights()
        if Cin != cw.dims.in_ch or H % 4 or W % 4:
            raise ValueError(f"expected (B, {cw.dims.in_ch}, 4k, 4m) images, got {tuple(x.shape)}")
        dev = x.device
        with torch.cuda.device(dev):
            ws, stream = self._c_workspace(L, cw, B, H, W, dev)
            vq = self.vector_quantization
            vws, prepared, key, slot = vq._workspace()
            if not prepared:
                slot[1] = None
            idx = torch.empty((B * (H // 4) * (W // 4), 1), dtype=torch.int64, device=dev)
            _lib.check(L.vqvae_encode_f32(cw, x.data_ptr(), B, H, W, (F_hip.VQ_CODEBOOK_PREPARED if prepared else 0) | vq_flags |
                                          (_cache.side(self)["c_scheme_hint"][0] if not (vq_flags & 0x3000) else 0),
                                          idx.data_ptr(), ws.data_ptr(), ws.numel(), vws.data_ptr(), vws.numel(), stream))
            slot[1] = key
        return idx

    def _decode_codes(self, idx, B, H, W, validate):
        """cosine_sim: rows of the normalised codebook (vq_decode_indices(idx, E^); vqvae_decode_f32 would gather un-normalised
        codes), then the decoder.  The no-grad forward and decode_indices both end here.  validate: raise on an index outside
        [0, K) (one host sync)."""
        from . import conv as C_hip
        z_q = F_hip.vq_decode_indices(idx.contiguous().view(-1).to(torch.int64), self.vector_quantization.normalized_codebook(),
                                      B, H, W, validate=validate)
        return C_hip.decoder_forward(self.decoder, z_q.detach(), rowmajor_in=False)

    def _decode_factorized(self, idx, B, H, W, validate, codebook=None):
        """codebook_dim: rows of the decoded codebook project_out(codes()) (vq_decode_indices(idx, codebook())), then the decoder.
        The no-grad forward and decode_indices both end here.  codebook: the decoded codebook the indices belong to, where it has
        moved since (the training-mode EMA forward)."""
        from . import conv as C_hip
        z_q = F_hip.vq_decode_indices(idx.contiguous().view(-1).to(torch.int64),
                                      codebook if codebook is not None else self.vector_quantization.codebook(), B, H, W,
                                      validate=validate)
        return C_hip.decoder_forward(self.decoder, z_q.detach(), rowmajor_in=False)

    def _decode_grouped(self, idx, B, H, W):
        """codebook_groups: the (G, N) indices' code rows side by side (functional.vq_grouped_decode), then the decoder.  The no-grad
        forward and decode_indices both end here."""
        from . import conv as C_hip
        vq = self.vector_quantization
        z_q = F_hip.vq_grouped_decode(idx, [w.detach() for w in vq.codebooks()], B, H, W, rowmajor=True, validate=False)
        return C_hip.decoder_forward(self.decoder, z_q, rowmajor_in=True)

    def _decode_fsq(self, idx, B, H, W, validate):
        """fsq_levels / lookup_free: the indices' rows (functional.fsq_decode_indices / lfq_decode_indices), then the decoder.  The
        no-grad forward and decode_indices both end here."""
        from . import conv as C_hip
        vq = self.vector_quantization
        if isinstance(vq, LookupFreeQuantizer):
            return C_hip.decoder_forward(self.decoder, vq.decode(idx, B, H, W, rowmajor=True, validate=validate), rowmajor_in=True)
        z_q = F_hip.fsq_decode_indices(idx.contiguous().view(-1).to(torch.int64), vq.project_out.weight.detach(),
                                       vq.project_out.bias.detach(), vq.levels, B, H, W, rowmajor=True, validate=validate)
        return C_hip.decoder_forward(self.decoder, z_q, rowmajor_in=True)

    @torch.no_grad()
    def decode_indices(self, idx, B, H, W, fwd_flags=None, validate=True):
        """indices -> x_hat (visualization.ipynb:358-365 generate_samples) as ONE call (vqvae_decode_f32): on the default shapes
        the decoder's first kernel takes every latent pixel's row straight from the codebook -- z_q is never written.
        H, W: the LATENT map's size.  Indices outside [0, K) raise, as the reference's one-hot scatter does -- that check reads
        idx.min() / idx.max() on the host (one sync per call); validate=False skips it for indices that come from encode(): the C
        entry never reads outside the codebook either way, a bad index shows as NaN pixels of its image (include/vqvae_hip.h)."""
        from . import _lib, conv as C_hip
        K = self.vector_quantization.n_e
        if isinstance(self.vector_quantization, ResidualVectorQuantizer):
            # n_quantizers * B * H * W indices, stage-major as encode() returns them: the sum of the stages' codes, then the decoder
            vq = self.vector_quantization
            if idx.numel() != vq.n_q * B * H * W:
                raise ValueError(f"expected {vq.n_q * B * H * W} indices ({vq.n_q} stages), got {idx.numel()}")
            idx = idx.contiguous().view(vq.n_q, -1).to(torch.int64)
            if validate and (int(idx.min()) < 0 or int(idx.max()) >= K):
                raise IndexError(f"code index out of range [0, {K})")
            z_q = F_hip.vq_residual_decode(idx, [w.detach() for w in vq.codebooks()], B, H, W, rowmajor=True,
                                           shared=vq.shared_codebook, validate=False)
            return C_hip.decoder_forward(self.decoder, z_q, rowmajor_in=True)
        if isinstance(self.vector_quantization, GroupedVectorQuantizer):
            # codebook_groups * B * H * W indices, group-major as encode() returns them
            vq = self.vector_quantization
            if idx.numel() != vq.n_g * B * H * W:
                raise ValueError(f"expected {vq.n_g * B * H * W} indices ({vq.n_g} groups), got {idx.numel()}")
            idx = idx.contiguous().view(vq.n_g, -1).to(torch.int64)
            if validate and (int(idx.min()) < 0 or int(idx.max()) >= K):
                raise IndexError(f"code index out of range [0, {K})")
            return self._decode_grouped(idx, B, H, W)
        if idx.numel() != B * H * W:
            raise ValueError(f"expected {B * H * W} indices, got {idx.numel()}")
        if isinstance(self.vector_quantization, (FiniteScalarQuantizer, LookupFreeQuantizer)):
            return self._decode_fsq(idx, B, H, W, validate=validate)
        if isinstance(self.vector_quantization, FactorizedVectorQuantizer):
            return self._decode_factorized(idx, B, H, W, validate=validate)
        if self.vector_quantization.cosine_sim:
            return self._decode_codes(idx, B, H, W, validate=validate)
        if C_hip.get_conv_backend() != "hip" or not idx.is_cuda:
            z_q = F_hip.vq_decode_indices(idx, self.vector_quantization.embedding.weight.detach(), B, H, W)
            return self.decoder(z_q)
        idx = _lib.dense(idx.contiguous().view(-1).to(torch.int64), 8)
        if validate and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= K):
            raise IndexError(f"code index out of range [0, {K})")
        L = _lib.load()
        cw, _keep = self._c_weights()
        if fwd_flags is None:
            fwd_flags = _cache.side(self)["c_scheme_hint"][0]
        dev = idx.device
        with torch.cuda.device(dev):
            ws, stream = self._c_workspace(L, cw, B, 4 * H, 4 * W, dev)
            x_hat = torch.empty((B, cw.dims.in_ch, 4 * H, 4 * W), dtype=torch.float32, device=dev)
            _lib.check(L.vqvae_decode_f32(cw, idx.data_ptr(), B, H, W, fwd_flags, x_hat.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return x_hat
