"""Host-side plumbing the fused optimizers (`AdamWScale`, `Adafactor`) share: the pinned ring their descriptor tables travel through
in eager steps, and the pre-capture arena + ownership token of a step recorded into a HIP graph.  No kernels, no arithmetic."""
import ctypes

import torch


class CapturedStepHost:
    """Mixin of a `torch.optim.Optimizer` whose `step()` launches through the C ABI.  Instance attributes (created lazily):
    `_staging` (upload rings), `_graph_arena` ({device: [uint8 tensor, bytes handed out]}), `_graph_jobs` / `_graph_keep` (what the
    captured step's launches read / must keep alive), `_capture_generation`."""

    def capture_token(self):
        """Ownership token of the captured step this optimizer currently holds (0: none).  Whoever captured keeps the token and hands it to
        `release_captured_step(token)`: a holder whose capture was already released -- and replaced by a newer one -- then releases nothing
        (an old GraphedTrainStep collected late must not clear the arena a live graph reads)."""
        return getattr(self, "_capture_generation", 0) if getattr(self, "_graph_jobs", None) else 0

    def release_captured_step(self, token=None):
        """Forget the captured step (the caller has destroyed every graph that holds it): its arena bytes may be handed out again.
        token (from `capture_token()` right after the capture): release only if the optimizer still holds THAT capture; None: unconditionally."""
        if token is not None and token != self.capture_token():
            return False
        self._graph_jobs, self._graph_keep = [], []
        for a in getattr(self, "_graph_arena", {}).values():
            a[1] = 0
        return True

    def _begin_capture(self):
        """first thing a `step()` under stream capture does.  ONE captured step per optimizer: the graph bakes raw pointers to the arena's
        descriptor table and step scalars into its launches, and graph_advance() writes the scalars of exactly one capture -- a second
        capture would hand the same arena bytes out again (the first graph would then replay over another table) and leave the first
        graph's scalars stale"""
        if getattr(self, "_graph_jobs", None):
            raise RuntimeError(f"{type(self).__name__}: this optimizer already holds a captured step; destroy that graph and call "
                               "release_captured_step() before capturing another one")
        self._graph_jobs, self._graph_keep = [], []
        self._capture_generation = getattr(self, "_capture_generation", 0) + 1  # (ownership token of THIS capture: capture_token())

    def _reserve_arena(self, need):
        """`need` = {device: bytes}: descriptor tables + step scalars of a captured step, one arena per device.  An arena a captured
        graph may be reading is never replaced or resized: it is allocated once and only while no step is captured."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return
        have = getattr(self, "_graph_arena", None)
        if have is None or any(dev not in have or have[dev][0].numel() < nb for dev, nb in need.items()):
            if getattr(self, "_graph_jobs", None):
                raise RuntimeError(f"{type(self).__name__}.init_state: parameters were added while a captured step exists; destroy that "
                                   "graph and call release_captured_step() first")
            self._graph_arena = {dev: [torch.empty(nb, dtype=torch.uint8, device=dev), 0] for dev, nb in need.items()}

    def _upload(self, device, table):
        """descriptor table -> device, ASYNCHRONOUSLY: through one of eight rotating pinned staging buffers (a copy from pageable memory
        makes the host wait for the stream, i.e. for the whole backward pass in front of it -- the host could never run ahead of the
        device).  A staging buffer is rewritten only after the copy issued from it eight uploads ago has completed."""
        n = ctypes.sizeof(table)
        ring = self.__dict__.setdefault("_staging", {}).setdefault(device, {"i": 0, "slot": 0, "pin": None, "ev": [None] * 8})
        if ring["pin"] is None or ring["slot"] < n:  # (ONE pinned allocation for the whole ring: hipHostMalloc costs milliseconds)
            for ev in ring["ev"]:
                if ev is not None:
                    ev.synchronize()
            ring["slot"] = max(2 * n, 1 << 16)
            ring["pin"] = torch.empty(8 * ring["slot"], dtype=torch.uint8).pin_memory()
            ring["ev"] = [None] * 8
        i = ring["i"]
        ring["i"] = (i + 1) % 8
        if ring["ev"][i] is not None:
            ring["ev"][i].synchronize()
        buf = ring["pin"][i * ring["slot"]:(i + 1) * ring["slot"]]
        ctypes.memmove(buf.data_ptr(), ctypes.addressof(table), n)
        raw = torch.empty(n, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            raw.copy_(buf[:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        ring["ev"][i] = ev
        return raw

    def _arena_take(self, device, nbytes):
        """`nbytes` of the pre-capture arena of `device` (64-byte aligned pieces, handed out in order)"""
        a = getattr(self, "_graph_arena", {}).get(device)
        if a is None:
            raise RuntimeError(f"{type(self).__name__}: call init_state() before capturing a step (it allocates the buffers a captured "
                               "step keeps outside the graph's memory pool)")
        off = a[1]
        a[1] = off + (nbytes + 63) // 64 * 64
        if a[1] > a[0].numel():
            raise RuntimeError(f"{type(self).__name__}: capture arena too small (parameters added after init_state()?)")
        return a[0][off:off + nbytes]
