"""Graph-replayed decode step for cached generation (`generate(..., cache_implementation="static", cross_attention_cache=True,
graph_decode=True)`).

A cached step over a StaticKVCache and a MediaCache is a few hundred small launches, each issued from Python: the host, not the GPU, bounds
it.  With the cache in replay mode (otter_amd/kv_cache.py) nothing in the step depends on the position on the
host side -- the position, the padding mask, the beam table and the running <image> counts are device buffers at fixed addresses -- so the
step is captured ONCE into a graph and every further step is one replay:

    prefill (eager, as always) -> enable_replay -> two eager replay-mode steps on the stream that will capture (they allocate every
    per-stream workspace in ordinary memory, build the rotary table to the cache's capacity, fill the kernels' CU-count cache and warm the
    library GEMM of the un-embedding) -> capture one step, static ids [rows, 1] -> static logits [rows, vocab] -> per step: copy the new
    ids in, reorder the two caches' small tables if there are beams (outside the graph, in place), replay.

The captured region is a single chain on a single stream (functional.single_chain: no side stream is forked inside).  The graph and its
private pool belong to one `generate` call and are released in its `finally` (`release`), together with this project's workspace entry
keyed by the capture stream (allocated by the warm-up steps in ordinary memory, never from the graph's pool).  Logits processing, sampling
and beam scoring stay eager, in otter_amd/generation.py.

On the CPU -- and wherever the cache's step does not run on csrc/decode_cache.hip (fp32 compute, other head sizes, grouped key / value
heads: `StaticKVCache.uses_kernel`, observed over the warm-up steps) -- there is no graph:
the same replay-mode step runs eagerly, which is what lets the CPU suite exercise the device-position bookkeeping end to end.
"""
from __future__ import annotations

import time

import torch

from . import functional as OF

WARMUP_STEPS = 2

# ONE capture stream per device, kept for the life of the process: what the libraries key by stream and keep for good (the library GEMM's
# workspace, 76 MiB per stream on this platform) is then allocated once, by the first call's warm-up steps, in ordinary memory -- a fresh
# stream per generate() call would add one such workspace per call.
_capture_streams = {}


def _capture_stream(device) -> "torch.cuda.Stream":
    key = device.index if device.index is not None else torch.cuda.current_device()
    st = _capture_streams.get(key)
    if st is None:
        st = _capture_streams[key] = torch.cuda.Stream(device=device)
    return st


class GraphDecodeStep:
    """The cached steps of one `generate` call.  `lm` is the decoder host (MPT / LLaMA with the Otter mixin), `cache` a prefilled
    StaticKVCache in replay mode, `media` the filled MediaCache.  Call it with the new ids [rows, 1]; it returns the logits [rows, vocab] of
    that step (from the third step on: the graph's static output buffer, valid until the next call).

    A host without a media cache (OtterHD / Fuyu-8B: otter_amd/fuyu.py) passes `media=None` and its own `step_fn(ids [rows, 1]) -> logits
    [rows, vocab]`, one replay-mode step over `cache`; `kernel_head_dim` is the head size at which that host's cached step runs on a HIP
    kernel (128: csrc/decode_cache.hip; 64: csrc/persimmon_decode_cache.hip)."""

    def __init__(self, lm, cache, media, step_fn=None, kernel_head_dim: int = 128):
        if not cache.replay:
            raise ValueError("GraphDecodeStep: the StaticKVCache must be in replay mode (enable_replay)")
        self.lm, self.cache, self.media = lm, cache, media
        if step_fn is not None:
            self._eager = step_fn
        if media is not None:
            media.fixed_address = True
        self.steps = self.captures = self.replays = 0
        self.capture_seconds = 0.0
        self.graph = self.logits = self.ids = self.stream = None
        # the graph needs every layer's step to be the HIP kernel's (StaticKVCache.uses_kernel: the plain-torch restatement reads the
        # position back to the host).  What the cache alone decides is decided here; the rest of that predicate (the query's dtype,
        # grouped key / value heads) is known after the warm-up steps, which the cache reports as `kernel_steps`.
        self.use_graph = cache.k.is_cuda and cache.dtype == torch.bfloat16 and cache.head_dim == kernel_head_dim
        if self.use_graph:
            self.ids = torch.zeros((cache.rows, 1), dtype=torch.long, device=cache.device)
            self.stream = _capture_stream(cache.device)

    def _eager(self, ids):
        out = self.lm(input_ids=ids, attention_mask=None, past_key_values=self.cache, use_cache=True, media_cache=self.media)
        return out.logits[:, -1, :]

    def __call__(self, new_ids: torch.Tensor) -> torch.Tensor:
        self.steps += 1
        if not self.use_graph:
            return self._eager(new_ids)
        self.ids.copy_(new_ids)
        if self.graph is not None:
            self.cache.note_replay()
            self.graph.replay()
            self.replays += 1
            return self.logits
        main = torch.cuda.current_stream(self.cache.device)
        if self.steps <= WARMUP_STEPS:
            self.stream.wait_stream(main)
            with torch.cuda.stream(self.stream):
                logits = self._eager(self.ids)
            main.wait_stream(self.stream)
            logits.record_stream(main)
            return logits
        if not self.cache.kernel_steps:             # a warm-up step ran the restatement: no capture, the eager replay-mode step goes on
            self.use_graph = False
            return self._eager(new_ids)
        torch.cuda.synchronize(self.cache.device)
        t0 = time.perf_counter()
        self.stream.wait_stream(main)
        graph = torch.cuda.CUDAGraph()
        with OF.single_chain(), torch.cuda.graph(graph, stream=self.stream):
            logits = self._eager(self.ids)          # (recorded, not run: the host length moved, the device position did not)
        self.graph, self.logits = graph, logits
        self.captures += 1
        torch.cuda.synchronize(self.cache.device)
        self.capture_seconds = time.perf_counter() - t0
        self.graph.replay()                         # the captured step itself: its device add brings pos_dev level with the host length
        self.replays += 1
        return self.logits

    def release(self) -> None:
        """Drop the graph, its private pool, the static buffers and the workspace entry keyed by the capture stream."""
        if self.graph is not None:
            torch.cuda.synchronize(self.cache.device)
            self.graph.reset()
        self.graph = self.logits = None
        if self.stream is not None:
            from . import ops

            ops._ws.drop_stream(self.cache.device, self.stream)
            self.stream = None
        self.ids = None
