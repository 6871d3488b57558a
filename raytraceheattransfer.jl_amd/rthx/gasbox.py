"""3D participating medium: a gas-filled box on the MI355X.

The reference has gas in 2D and surface enclosures in 3D; this is the missing
quadrant in its simplest form, the furnace box of the zone method: an
axis-aligned box of n[0] x n[1] x n[2] uniform cells filled with one grey
medium (kappa, sigma_s), all six faces walls.  Exchange factors are traced by
librthx (rthx_gasbox_trace, csrc/rthx_gasbox_kernels.hip); smoothing and the
grey solve are the ones every other domain uses (rthx_smooth_F_result,
rthx_solve_grey_smoothed).  VoxelGasBox3D is the same box with kappa and
sigma_s given per voxel: its rays walk the lattice
(rthx_gasbox_trace_field, csrc/rthx_gasbox_field_kernels.hip).  No CPU
fallback.

Element order (include/rthx.h): surfaces first, faces f = 2 axis + side (x-,
x+, y-, y+, z-, z+), on a face of axis a with the other axes p < q cell
(c_p, c_q) at face_offset[f] + c_p + n_p c_q; then volumes, (c_x, c_y, c_z) at
Ns + c_x + n_x (c_y + n_y c_z).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import scipy.sparse as sp

from . import abi


def _other_axes(a: int):
    return [k for k in range(3) if k != a]


class GasBox3D:
    """The box lo < hi with n cells per axis and one grey medium.

    Wall properties (epsilon, T_in_w [K], q_in_w [W per element]) are a
    scalar, one value per face (6) or one per surface element (Ns); gas
    properties (T_in_g, q_in_g [W per voxel]) a scalar or one per volume.
    kappa and sigma_s are scalars: the medium is uniform.  A negative T means
    "in radiative equilibrium, q given", as everywhere else."""

    def __init__(self, lo, hi, n, kappa, sigma_s=0.0, epsilon=1.0, T_in_w=0.0, q_in_w=0.0, T_in_g=-1.0,
                 q_in_g=0.0):
        self.lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1)
        self.hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(-1)
        self.n = np.ascontiguousarray(n, dtype=np.int32).reshape(-1)
        if self.lo.size != 3 or self.hi.size != 3 or self.n.size != 3:
            raise ValueError("lo, hi and n have three entries each")
        if np.ndim(kappa) != 0 or np.ndim(sigma_s) != 0:
            raise ValueError("kappa and sigma_s are scalars: the gas box holds one uniform medium")
        self.kappa, self.sigma_s = float(kappa), float(sigma_s)
        if not (self.kappa >= 0.0 and self.sigma_s >= 0.0):
            raise ValueError("kappa and sigma_s must be >= 0")
        lay = self.layout()  # (checks n through the library)
        self.n_surfaces, self.n_volumes = lay["n_surfaces"], lay["n_volumes"]
        self.num_elements = self.n_surfaces + self.n_volumes
        self.face_offset = lay["face_offset"]
        self.epsilon = self._per_wall(epsilon, "epsilon")
        self.T_in_w = self._per_wall(T_in_w, "T_in_w")
        self.q_in_w = self._per_wall(q_in_w, "q_in_w")
        self.T_in_g = self._per_volume(T_in_g, "T_in_g")
        self.q_in_g = self._per_volume(q_in_g, "q_in_g")
        self.device = 0
        self._handles: dict = {}
        self._result = None
        self._F_raw = None
        self._F_smooth = None
        self.F_smooth_handle = None
        self.last_trace_info: dict = {}
        self.last_smooth_info: dict = {}
        self.last_solve_info: dict = {}
        self.T_w = self.q_w = self.T_g = self.q_g = None
        self.energy_error = None

    # ---- element bookkeeping -------------------------------------------------
    @property
    def beta(self) -> float:
        return self.kappa + self.sigma_s

    def _per_wall(self, v, name):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            return np.full(self.n_surfaces, float(a))
        a = a.reshape(-1)
        if a.size == self.n_surfaces:  # (n = (1, 1, 1): a face is an element)
            return a.copy()
        if a.size == 6:
            return np.repeat(a, np.diff(self.face_offset))
        raise ValueError(f"{name}: a scalar, 6 face values or {self.n_surfaces} surface values")

    def _per_volume(self, v, name):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            return np.full(self.n_volumes, float(a))
        a = a.reshape(-1)
        if a.size != self.n_volumes:
            raise ValueError(f"{name}: a scalar or {self.n_volumes} volume values")
        return a.copy()

    def layout(self) -> dict:
        """rthx_gasbox_layout (host only): n_surfaces, n_volumes, n_elements
        and face_offset[7]."""
        from ._lib import check, load

        ns, nv = C.c_int64(0), C.c_int64(0)
        off = np.zeros(7, dtype=np.int64)
        check(load().rthx_gasbox_layout(abi.ptr(self.n, C.c_int32), C.byref(ns), C.byref(nv), abi.ptr(off, C.c_int64)))
        return {"n_surfaces": ns.value, "n_volumes": nv.value, "n_elements": ns.value + nv.value, "face_offset": off}

    @property
    def h(self) -> np.ndarray:
        return (self.hi - self.lo) / self.n

    def polygon_arrays(self):
        """The wall quads in element order: (xyz[Ns][4][3], nv[Ns] = 4,
        normals[Ns][3]), the normals pointing into the box and each quad's
        vertices counter-clockwise about its normal."""
        h = self.h
        xyz = np.zeros((self.n_surfaces, 4, 3))
        normals = np.zeros((self.n_surfaces, 3))
        k = 0
        for f in range(6):
            a, side = f >> 1, f & 1
            p, q = _other_axes(a)
            plane = self.hi[a] if side else self.lo[a]
            corners = [(0, 0), (1, 0), (1, 1), (0, 1)]
            # e_p x e_q is +e_a for a = 0, 2 and -e_a for a = 1; the inward normal is +e_a on side 0
            if (a == 1) != (side == 1):
                corners = corners[::-1]
            for cq in range(self.n[q]):
                for cp in range(self.n[p]):
                    for v, (ip, iq) in enumerate(corners):
                        xyz[k, v, a] = plane
                        xyz[k, v, p] = self.lo[p] + (cp + ip) * h[p]
                        xyz[k, v, q] = self.lo[q] + (cq + iq) * h[q]
                    normals[k, a] = -1.0 if side else 1.0
                    k += 1
        return xyz, np.full(self.n_surfaces, 4, dtype=np.int32), normals

    def areas(self) -> np.ndarray:
        h = self.h
        per_face = [h[_other_axes(f >> 1)[0]] * h[_other_axes(f >> 1)[1]] for f in range(6)]
        return np.repeat(per_face, np.diff(self.face_offset))

    def volume(self) -> float:
        return float(np.prod(self.h))

    def weights(self) -> np.ndarray:
        """get_w's rule (smoothExchangeFactors.jl:320-341): wall areas, then
        max(1e-6, 4 beta V) for every volume."""
        return np.concatenate([self.areas(), np.full(self.n_volumes, max(1e-6, 4.0 * self.beta * self.volume()))])

    # ---- device ----------------------------------------------------------------
    def _handle(self, device: int):
        from ._lib import check, load

        h = self._handles.get(device)
        if h is None:
            h = C.c_void_p()
            check(load().rthx_gasbox_create(abi.ptr(self.lo, C.c_double), abi.ptr(self.hi, C.c_double),
                                            abi.ptr(self.n, C.c_int32), device, C.byref(h)))
            self._handles[device] = h
        return h

    def trace(self, rays_per_emitter: int, seed: int = 1, faithful: bool = False, ray_begin: int = 0,
              emitter_begin: int = 0, emitter_end: Optional[int] = None, emitter_stride: int = 1, result=None,
              device: Optional[int] = None, beta: Optional[float] = None):
        """rthx_gasbox_trace into a DeviceResult (returned; `result`: one to
        reuse) whose counts stay on the device: csr(), F(), accumulate(),
        sampling_error(), torch_csr() and the device smoothing read them
        there.  `beta` overrides kappa + sigma_s (one trace per band)."""
        from ._lib import DeviceResult, check, load, make_args

        dev = self.device if device is None else int(device)
        flags = (abi.RTHX_FLAG_FAITHFUL_SAMPLING if faithful else 0) | abi.RTHX_FLAG_DEVICE_ONLY
        args, _keep = make_args(0, rays_per_emitter, 0.0, seed, emitter_begin,
                                self.num_elements if emitter_end is None else emitter_end, emitter_stride, dev, flags)
        res = DeviceResult() if result is None else result
        try:
            check(load().rthx_gasbox_trace(self._handle(dev), C.byref(args), float(self.beta if beta is None else beta),
                                           int(ray_begin), res.handle))
        except Exception:
            if result is None:
                res.close()
            raise
        return res

    # The orthogonal projection of smooth_F (its Dykstra rounds) works on dense
    # N x N matrices, several at a time: above this N the box leaves the choice
    # to smooth_F's own rule (sparse alternating projection unless F is dense).
    DENSE_SMOOTH_MAX_N = 16384

    def __call__(self, rays_tot: int, seed: int = 1, device: int = 0, max_iters: int = 1000, verbose: bool = False,
                 k_dykstra: Optional[int] = None):
        """Traces rays_tot // N rays per emitter and smooths the counts where
        they lie (smooth_F_device with weights() and Ns).  Afterwards F_raw
        and F_smooth read the two matrices (host copies made on first
        access) and F_smooth_handle is the device-resident F_smooth that
        solve_equilibrium reads in place.

        k_dykstra: Dykstra rounds of smooth_F.  None: one round (the
        reference's orthogonal projection OP before the alternating
        projection) up to DENSE_SMOOTH_MAX_N elements, smooth_F's automatic
        choice beyond.  Why not the automatic choice throughout: without OP
        smooth_F starts from X = (W F + (W F)')/2, the plain mean of the two
        estimates x_ij = w_i F_ij and x_ji = w_j F_ji of one exchange flux.
        With R rays a row their variances are x w_i / R and x w_j / R, and a
        wall's weight (its area) and a voxel's (4 beta V) differ by orders of
        magnitude in a thin gas: a wall row sends few rays into the gas, and
        the mean keeps half of their noise.  OP weights the pair by
        w_j^2 : w_i^2, the estimate from the lighter element most; its
        variance over the mean's is 4 t (1 - t) with t = w_i w_j / (w_i^2 +
        w_j^2), never above 1 and small where the weights differ.  smooth_F's
        own switch (cross coupling chi >= 0.4) reads the mass of F_raw's
        wall-gas blocks, which a thin gas on a coarse lattice (Nv / N < 0.4)
        does not reach."""
        from .smoothing import smooth_F_device

        self.device = int(device)
        R = max(1, int(rays_tot) // self.num_elements)
        self._drop_matrices()
        self._result = self.trace(R, seed=seed, device=device)
        self.last_trace_info = self._result.info()
        if k_dykstra is None and self.num_elements <= self.DENSE_SMOOTH_MAX_N:
            k_dykstra = 1
        info: dict = {}
        self.F_smooth_handle = smooth_F_device(self._result, self.num_elements, self.weights(), self.n_surfaces,
                                               max_iters=max_iters, k_dykstra=k_dykstra, verbose=verbose, device=device,
                                               info=info)
        self.last_smooth_info = info
        return None

    def _drop_matrices(self) -> None:
        if self.F_smooth_handle is not None:
            self.F_smooth_handle.close()
        if self._result is not None:
            self._result.close()
        self.F_smooth_handle = self._result = self._F_raw = self._F_smooth = None

    @property
    def F_raw(self):
        """counts / R, row-normalised on the device, as scipy CSR."""
        if self._F_raw is None and self._result is not None:
            rp, cols, vals = self._result.F()
            self._F_raw = sp.csr_matrix((vals, cols, rp), shape=(self.num_elements,) * 2)
        return self._F_raw

    @property
    def F_smooth(self):
        if self._F_smooth is None and self.F_smooth_handle is not None:
            self._F_smooth = self.F_smooth_handle.host()
        return self._F_smooth

    def close(self) -> None:
        self._drop_matrices()
        if self._handles:
            from ._lib import load

            for h in self._handles.values():
                load().rthx_gasbox_destroy(h)
            self._handles = {}

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class VoxelGasBox3D(GasBox3D):
    """The box with one grey medium per voxel: a flame core, a cooler shell,
    soot layers.

    kappa and sigma_s are each a scalar, n_volumes values in element order
    (c_x fastest) or an array of shape (n_x, n_y, n_z) indexed
    [c_x, c_y, c_z]; both are kept per voxel, in element order, and beta is
    their sum.  Everything else is GasBox3D's.  Rays are traced by
    rthx_gasbox_trace_field, which crosses the lattice cell by cell; voxels
    with beta = 0 are legal in trace() and absorb nothing, but __call__
    refuses them: a transparent voxel exchanges no heat and would have to
    leave the system that is smoothed and solved."""

    def __init__(self, lo, hi, n, kappa, sigma_s=0.0, epsilon=1.0, T_in_w=0.0, q_in_w=0.0, T_in_g=-1.0,
                 q_in_g=0.0):
        super().__init__(lo, hi, n, 0.0, 0.0, epsilon=epsilon, T_in_w=T_in_w, q_in_w=q_in_w, T_in_g=T_in_g,
                         q_in_g=q_in_g)
        self.kappa = self._field(kappa, "kappa")
        self.sigma_s = self._field(sigma_s, "sigma_s")

    def _field(self, v, name) -> np.ndarray:
        """A scalar, n_volumes values in element order or an (n_x, n_y, n_z)
        array -> n_volumes values in element order, finite and >= 0."""
        a = np.asarray(v, dtype=np.float64)
        shape = tuple(int(k) for k in self.n)
        if a.ndim == 0:
            out = np.full(self.n_volumes, float(a))
        elif a.ndim == 3 and a.shape == shape:
            out = a.transpose(2, 1, 0).reshape(-1).copy()  # [c_x, c_y, c_z] -> c_x + n_x (c_y + n_y c_z)
        elif a.ndim == 1 and a.size == self.n_volumes:
            out = a.copy()
        else:
            raise ValueError(f"{name}: a scalar, {self.n_volumes} volume values in element order or an array of "
                             f"shape {shape}")
        if not (np.all(np.isfinite(out)) and np.all(out >= 0.0)):
            raise ValueError(f"{name} must be finite and >= 0 in every voxel")
        return out

    @property
    def beta(self) -> np.ndarray:
        return self.kappa + self.sigma_s

    def weights(self) -> np.ndarray:
        """Wall areas, then max(1e-6, 4 beta_v V) per volume (get_w's rule,
        voxel by voxel)."""
        return np.concatenate([self.areas(), np.maximum(1e-6, 4.0 * self.beta * self.volume())])

    def trace(self, rays_per_emitter: int, seed: int = 1, faithful: bool = False, ray_begin: int = 0,
              emitter_begin: int = 0, emitter_end: Optional[int] = None, emitter_stride: int = 1, result=None,
              device: Optional[int] = None, beta=None):
        """rthx_gasbox_trace_field into a DeviceResult, as GasBox3D.trace.
        `beta` overrides the field kappa + sigma_s (a scalar, element order or
        [c_x, c_y, c_z]; one trace per band)."""
        from ._lib import DeviceResult, check, load, make_args

        dev = self.device if device is None else int(device)
        flags = (abi.RTHX_FLAG_FAITHFUL_SAMPLING if faithful else 0) | abi.RTHX_FLAG_DEVICE_ONLY
        args, _keep = make_args(0, rays_per_emitter, 0.0, seed, emitter_begin,
                                self.num_elements if emitter_end is None else emitter_end, emitter_stride, dev, flags)
        field = np.ascontiguousarray(self.beta if beta is None else self._field(beta, "beta"), dtype=np.float64)
        res = DeviceResult() if result is None else result
        try:
            check(load().rthx_gasbox_trace_field(self._handle(dev), C.byref(args), abi.ptr(field, C.c_double),
                                                 field.size, int(ray_begin), res.handle))
        except Exception:
            if result is None:
                res.close()
            raise
        return res

    def __call__(self, rays_tot: int, seed: int = 1, device: int = 0, max_iters: int = 1000, verbose: bool = False,
                 k_dykstra: Optional[int] = None):
        if np.any(self.beta == 0.0):
            raise ValueError("a voxel with beta = 0 takes no part in the exchange: smoothing and the solve need "
                             "beta > 0 in every voxel (trace() accepts such a field)")
        return super().__call__(rays_tot, seed=seed, device=device, max_iters=max_iters, verbose=verbose,
                                k_dykstra=k_dykstra)
