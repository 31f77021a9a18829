"""hipGraph replay of the forward path for launch-bound batch sizes.

At BASELINE config 1 (B=32) the ~20 kernels of `VQVAE.forward` run for a few tens of microseconds in total,
less than the host needs to launch them one by one.  `GraphedForward` captures one forward on a private
stream into a hipGraph (through `torch.cuda.CUDAGraph`, i.e. hipStreamBeginCapture / hipGraphLaunch on ROCm)
and replays it with a single launch; every kernel in the graph is still ours (libvqvae_hip.so), torch only
provides the capture, the static buffers and the stream.

    g = GraphedForward(model, example_x)         # warms up, captures
    embedding_loss, x_hat, perplexity = g(x)     # copies x into the static input, replays, returns the
                                                 # static outputs (valid until the next call; .clone() to keep)

Shapes are fixed at capture time; weights are read through their device pointers, so in-place weight updates
are seen by later replays, but the packed-weight / codebook images are only rebuilt by an eager call
(re-capture after changing parameters).  Forward-only, CUDA(HIP) fp32 tensors only, no fallback.

`GraphedStep` does the same for a whole training step (zero_grad, forward, losses, backward, optimizer step):

    def step(x):
        opt.zero_grad(set_to_none=False); el, xh, pp = model(x)
        stats = training.step_losses(el, xh, pp, x, var); stats[1].backward(); opt.step(); return stats
    g = GraphedStep(model, step, example_x)      # `warmup` REAL steps on the capture stream, then the capture
    stats = g(x)                                 # copy, replay, and the version counters of the model's state advance

A replay runs no Python: the kernels move the weights, the EMA buffers and the optimizer state through their device pointers, and
the `_version` bumps that `optim.Adam.step` and the EMA update make in Python do not happen.  Every packed-weight and codebook
cache of this package is keyed on (data_ptr, _version); an eager call after a raw `graph.replay()` would therefore reuse images
packed from older weights.  `GraphedStep` advances the `_version` of every parameter and buffer of the model after each replay;
whoever replays a graph of their own calls `model.invalidate_caches()` before the next eager use of the model.
"""
from __future__ import annotations

import torch

from . import _lib


class GraphedForward:
    def __init__(self, model, example_x, warmup: int = 3):
        if not example_x.is_cuda:
            raise _lib.VqvaeHipError("GraphedForward needs a CUDA(HIP) example input: there is no CPU path")
        _lib.load()
        _lib.profile_enable(False)               # event records are not capturable work we want in the graph
        self.model = model
        self.static_x = example_x.detach().clone().contiguous()
        self._stream = torch.cuda.Stream(device=example_x.device)
        self._graph = torch.cuda.CUDAGraph()
        with torch.no_grad():
            # eager warm-up on the capture stream: packs weights, prepares the codebook image, sets kernel
            # attributes and fills the allocator's pools, none of which may happen inside the capture
            self._stream.wait_stream(torch.cuda.current_stream(example_x.device))
            with torch.cuda.stream(self._stream):
                for _ in range(max(1, warmup)):
                    out = model(self.static_x)
            self._stream.synchronize()
            with torch.cuda.graph(self._graph, stream=self._stream):
                out = model(self.static_x)
        self.static_out = out

    def __call__(self, x):
        if x.shape != self.static_x.shape or x.dtype != self.static_x.dtype:
            raise ValueError(f"graph captured for {tuple(self.static_x.shape)} {self.static_x.dtype}, "
                             f"got {tuple(x.shape)} {x.dtype}")
        self.static_x.copy_(x, non_blocking=True)
        self._graph.replay()
        return self.static_out

    def replay(self):
        """Replay on whatever is in `static_x` (no input copy)."""
        self._graph.replay()
        return self.static_out


class GraphedStep:
    """One training step, captured once and replayed.  `step(*static_inputs)` must do all of its work on the current stream, on
    static tensors (gradients included: `zero_grad(set_to_none=False)`), and may return tensors (the static outputs).  The `warmup`
    eager calls before the capture are real steps: the weights and the optimizer state move."""

    def __init__(self, model, step, *example_inputs, warmup: int = 3):
        if not example_inputs or not all(t.is_cuda for t in example_inputs):
            raise _lib.VqvaeHipError("GraphedStep needs CUDA(HIP) example inputs: there is no CPU path")
        for mod in model.modules():
            if getattr(mod, "_ema_merging", False):
                # the pending count, the collective and the decision to apply are Python state: a replay would run none of it
                raise _lib.VqvaeHipError("GraphedStep captures one forward, not a cycle of the EMA quantizer's sync / accumulate "
                                         "options (ema_sync, ema_accumulate): step such a model eagerly")
        _lib.load()
        _lib.profile_enable(False)
        self.model = model
        self.static_inputs = tuple(t.detach().clone().contiguous() for t in example_inputs)
        dev = example_inputs[0].device
        self._stream = torch.cuda.Stream(device=dev)
        self._graph = torch.cuda.CUDAGraph()
        # eager steps on the capture stream: the gradient tensors, the optimizer's plan, every workspace and the allocator's pools
        # exist afterwards, none of which may come into being inside the capture
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self._stream):
            for _ in range(max(1, warmup)):
                step(*self.static_inputs)
        self._stream.synchronize()
        with torch.cuda.graph(self._graph, stream=self._stream):
            self.static_out = step(*self.static_inputs)
        self._written = list(model.parameters()) + list(model.buffers())

    def __call__(self, *inputs):
        if len(inputs) != len(self.static_inputs):
            raise ValueError(f"graph captured for {len(self.static_inputs)} inputs, got {len(inputs)}")
        for s, x in zip(self.static_inputs, inputs):
            if x.shape != s.shape or x.dtype != s.dtype:
                raise ValueError(f"graph captured for {tuple(s.shape)} {s.dtype}, got {tuple(x.shape)} {x.dtype}")
        for s, x in zip(self.static_inputs, inputs):
            s.copy_(x, non_blocking=True)
        return self.replay()

    def replay(self):
        """Replay on whatever is in `static_inputs` (no input copy)."""
        self._graph.replay()
        # what the step's Python did and a replay does not: the caches keyed on (data_ptr, _version) must see the new weights
        torch.autograd.graph.increment_version(self._written)
        return self.static_out
