"""Progressive exchange traces: extend a trace by further rays and stop on
its sampling error.

Every ray is a pure function of (seed, bin, emitter, ray id), so a trace of
R rays per emitter can be continued: ``ProgressiveTrace.extend(r)`` traces
the ray ids [R, R + r) of every emitter (rthx_trace_exchange_rays) into a
scratch result and adds its counts to the ones held on the device
(rthx_result_accumulate).  The counts after any sequence of extensions are
those of one trace of the summed rays, bit for bit.
``sampling_error()`` is the binomial error of F_raw = count / tallied
(rthx_result_sampling_error); ``trace_to_tolerance`` extends in batches until
its rms reaches a tolerance.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import abi
from ._lib import DeviceResult, device_domain, make_args


class ProgressiveTrace:
    """The counts of one bin of `dom` on `device`, extendable by rays."""

    def __init__(self, dom, spectral_bin: int = 1, nudge: Optional[float] = None, seed: int = 1, device: int = 0,
                 faithful: bool = False):
        self.dom = dom
        self.bin0 = spectral_bin - 1
        self.nudge = 10_000 * np.finfo(np.float64).eps if nudge is None else nudge
        self.seed = seed
        self.device = device
        self.faithful = faithful
        self.n = dom.flat().n_emitters
        self._dd = device_domain(dom, device)
        self._res: Optional[DeviceResult] = None  # the accumulated counts
        self._scratch: Optional[DeviceResult] = None
        self.rays_per_emitter = 0
        self.accumulate_ms = 0.0  # device time of the accumulates so far

    def _args(self, rays: int):
        flags = abi.RTHX_FLAG_DEVICE_ONLY | (abi.RTHX_FLAG_FAITHFUL_SAMPLING if self.faithful else 0)
        return make_args(self.bin0, rays, self.nudge, self.seed, 0, self.n, 1, self.device, flags)

    def extend(self, rays_per_emitter: int) -> "ProgressiveTrace":
        """Trace the next `rays_per_emitter` ray ids of every emitter and add
        their counts."""
        r = int(rays_per_emitter)
        if r < 0:
            raise ValueError("rays_per_emitter must not be negative")
        args, keep = self._args(r)
        if self._res is None:
            self._res = DeviceResult().trace(self._dd, args, ray_begin=self.rays_per_emitter)
        else:
            if self._scratch is None:
                self._scratch = DeviceResult()
            self._scratch.trace(self._dd, args, ray_begin=self.rays_per_emitter)
            self._res.accumulate(self._scratch)
            self.accumulate_ms += self._res.accumulate_ms()
        del keep
        self.rays_per_emitter += r
        return self

    @property
    def device_result(self) -> DeviceResult:
        """The accumulated counts (for rthx_smooth_F_result, torch_csr, ...)."""
        if self._res is None:
            raise RuntimeError("nothing traced yet: call extend() first")
        return self._res

    def info(self) -> dict:
        return self.device_result.info()

    def csr(self):
        """(row_ptr, cols, counts) on the host."""
        return self.device_result.csr()

    def F(self):
        """F_raw = count / tallied as CSR (row_ptr, cols, vals) on the host."""
        return self.device_result.F()

    def sampling_error(self) -> Tuple[float, float]:
        """(rms, max_row) of the binomial sampling error of F_raw."""
        return self.device_result.sampling_error()

    def close(self) -> None:
        for r in (self._res, self._scratch):
            if r is not None:
                r.close()
        self._res = self._scratch = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def trace_to_tolerance(dom, rms_tol: float, batch: int, max_rays_per_emitter: int, spectral_bin: int = 1,
                       nudge: Optional[float] = None, seed: int = 1, device: int = 0, faithful: bool = False):
    """Extend a trace of `dom` in batches of `batch` rays per emitter until
    the rms sampling error is at or under `rms_tol` or `max_rays_per_emitter`
    is reached (the last batch is cut to the cap).  Returns (trace, history)
    with history the list of (rays per emitter, rms) after every batch."""
    if batch < 1:
        raise ValueError("batch must be positive")
    t = ProgressiveTrace(dom, spectral_bin, nudge, seed, device, faithful)
    history: List[Tuple[int, float]] = []
    try:
        while t.rays_per_emitter < max_rays_per_emitter:
            t.extend(min(batch, max_rays_per_emitter - t.rays_per_emitter))
            rms, _ = t.sampling_error()
            history.append((t.rays_per_emitter, rms))
            if rms <= rms_tol:
                break
    except Exception:
        t.close()
        raise
    return t, history
