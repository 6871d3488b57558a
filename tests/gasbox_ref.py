"""Independent restatement of the 3D gas-box tracer (include/rthx.h
rthx_gasbox_*) for the tests: element layout and geometry, a
numpy Monte Carlo trace with numpy's own generator, and Gauss-Legendre
quadrature of the four kinds of exchange integral.  Nothing here reads the
library or shares code with it.

Elements: surfaces first -- faces f = 2 axis + side (x-, x+, y-, y+, z-, z+),
on a face of axis a with the other axes p < q cell (c_p, c_q) at
face_offset[f] + c_p + n_p c_q -- then volumes, (c_x, c_y, c_z) at
Ns + c_x + n_x (c_y + n_y c_z).
"""
from __future__ import annotations

import numpy as np


def other_axes(a):
    return [k for k in range(3) if k != a]


class Box:
    def __init__(self, lo, hi, n):
        self.lo = np.asarray(lo, dtype=np.float64)
        self.hi = np.asarray(hi, dtype=np.float64)
        self.n = np.asarray(n, dtype=np.int64)
        self.h = (self.hi - self.lo) / self.n
        off = [0]
        for f in range(6):
            p, q = other_axes(f >> 1)
            off.append(off[-1] + int(self.n[p] * self.n[q]))
        self.face_offset = np.array(off, dtype=np.int64)
        self.Ns = off[-1]
        self.Nv = int(np.prod(self.n))
        self.N = self.Ns + self.Nv

    # -- elements -----------------------------------------------------------
    def wall_index(self, f, cp, cq):
        p, _q = other_axes(f >> 1)
        return int(self.face_offset[f] + cp + self.n[p] * cq)

    def volume_index(self, cx, cy, cz):
        return int(self.Ns + cx + self.n[0] * (cy + self.n[1] * cz))

    def element(self, g):
        """('wall', f, (cp, cq)) or ('vol', None, (cx, cy, cz))."""
        if g >= self.Ns:
            v = g - self.Ns
            return "vol", None, (v % self.n[0], (v // self.n[0]) % self.n[1], v // (self.n[0] * self.n[1]))
        f = int(np.searchsorted(self.face_offset, g, side="right") - 1)
        p, _q = other_axes(f >> 1)
        loc = g - self.face_offset[f]
        return "wall", f, (loc % self.n[p], loc // self.n[p])

    def bounds(self, g):
        """Bounding box (lo[3], hi[3]) of element g; a wall is flat along its axis."""
        kind, f, c = self.element(g)
        if kind == "vol":
            c = np.array(c)
            return self.lo + c * self.h, self.lo + (c + 1) * self.h
        a, side = f >> 1, f & 1
        p, q = other_axes(a)
        lo, hi = np.zeros(3), np.zeros(3)
        lo[a] = hi[a] = self.hi[a] if side else self.lo[a]
        for ax, ci in ((p, c[0]), (q, c[1])):
            lo[ax] = self.lo[ax] + ci * self.h[ax]
            hi[ax] = self.lo[ax] + (ci + 1) * self.h[ax]
        return lo, hi

    def inward_normal(self, f):
        nrm = np.zeros(3)
        nrm[f >> 1] = -1.0 if (f & 1) else 1.0
        return nrm

    def size(self, g):
        """Area of a wall cell, volume of a voxel."""
        lo, hi = self.bounds(g)
        ext = hi - lo
        return float(np.prod(ext[ext > 0]))

    def separated(self, i, j):
        """A gap of at least one cell between the two elements along some axis."""
        li, hi_ = self.bounds(i)
        lj, hj = self.bounds(j)
        gap = np.maximum(li - hj, lj - hi_)
        return bool(np.any(gap >= self.h * (1.0 - 1e-9)))

    # -- Monte Carlo ----------------------------------------------------------
    def trace_row(self, g, R, beta, rng):
        """Absorber counts [N] of R rays from emitter g."""
        kind, f, c = self.element(g)
        lo_e, hi_e = self.bounds(g)
        o = lo_e + rng.random((R, 3)) * (hi_e - lo_e)
        phi = 2.0 * np.pi * rng.random(R)
        u = rng.random(R)
        d = np.empty((R, 3))
        if kind == "wall":
            a, side = f >> 1, f & 1
            p, q = other_axes(a)
            ct, st = np.sqrt(1.0 - u), np.sqrt(u)
            d[:, a] = -ct if side else ct
            d[:, p] = st * np.cos(phi)
            d[:, q] = st * np.sin(phi)
        else:
            ct = 1.0 - 2.0 * u
            st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
            d[:, 0] = st * np.cos(phi)
            d[:, 1] = st * np.sin(phi)
            d[:, 2] = ct
        S = -np.log(1.0 - rng.random(R)) / beta if beta > 0 else np.full(R, np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_ax = np.where(d == 0.0, np.inf, (np.where(d > 0.0, self.hi, self.lo) - o) / d)
        ax = np.argmin(t_ax, axis=1)  # (the first minimum: the lowest axis on a tie)
        t = t_ax[np.arange(R), ax]
        gas = S < t
        end = o + np.where(gas, S, t)[:, None] * d
        cell = np.clip(np.floor((end - self.lo) / self.h).astype(np.int64), 0, self.n - 1)
        cols = self.Ns + cell[:, 0] + self.n[0] * (cell[:, 1] + self.n[1] * cell[:, 2])
        face = 2 * ax + (d[np.arange(R), ax] > 0.0)
        for a in range(3):
            p, q = other_axes(a)
            m = ~gas & (ax == a)
            cols[m] = self.face_offset[face[m]] + cell[m, p] + self.n[p] * cell[m, q]
        return np.bincount(cols, minlength=self.N)

    def trace(self, rows, R, beta, seed):
        rng = np.random.default_rng(seed)
        return np.array([self.trace_row(int(g), R, beta, rng) for g in rows])

    # -- quadrature -------------------------------------------------------------
    def nodes(self, g, m=8):
        """Gauss-Legendre points [k, 3] and weights [k] over element g (m per
        dimension; the weights sum to its area or volume)."""
        x, w = np.polynomial.legendre.leggauss(m)
        x, w = 0.5 * (x + 1.0), 0.5 * w
        lo, hi = self.bounds(g)
        axes = [k for k in range(3) if hi[k] > lo[k]]
        grids = np.meshgrid(*[x] * len(axes), indexing="ij")
        wg = np.meshgrid(*[w] * len(axes), indexing="ij")
        pts = np.tile(lo, (grids[0].size, 1))
        wt = np.ones(grids[0].size)
        for k, ax in enumerate(axes):
            pts[:, ax] = lo[ax] + grids[k].ravel() * (hi[ax] - lo[ax])
            wt *= wg[k].ravel() * (hi[ax] - lo[ax])
        return pts, wt

    def pair_integral(self, i, j, beta, m=8):
        """F_ij by quadrature.  With r between the integration points and the
        cosines at the walls' inward normals:
          volume -> volume    (1/V_i) int int beta e^{-beta r} / (4 pi r^2) dV_j dV_i
          volume -> surface   (1/V_i) int int cos_j e^{-beta r} / (4 pi r^2) dA_j dV_i
          surface -> volume   (1/A_i) int int cos_i beta e^{-beta r} / (pi r^2) dV_j dA_i
          surface -> surface  (1/A_i) int int cos_i cos_j e^{-beta r} / (pi r^2) dA_j dA_i"""
        ki, fi, _ = self.element(i)
        kj, fj, _ = self.element(j)
        Pi, wi = self.nodes(i, m)
        Pj, wj = self.nodes(j, m)
        D = Pj[None, :, :] - Pi[:, None, :]
        r = np.sqrt(np.sum(D * D, axis=2))
        k = np.exp(-beta * r) / (r * r)
        if ki == "wall":
            k = k * np.maximum(0.0, D @ self.inward_normal(fi)) / r / np.pi
        else:
            k = k / (4.0 * np.pi)
        if kj == "wall":
            k = k * np.maximum(0.0, -(D @ self.inward_normal(fj))) / r
        else:
            k = k * beta
        return float(wi @ k @ wj) / self.size(i)

    def volume_to_face(self, v, f, beta, m_out=24, m_corr=8):
        """F(voxel v -> the whole face f), touching pairs included.  The face
        integral of cos e^{-beta r} / (4 pi r^2) is split into the solid angle
        of the face's rectangle over 4 pi (closed form, A. Van Oosterom and
        J. Strackee, IEEE Trans. Biomed. Eng. 30 (1983) for the triangle; the
        arctangent form for a rectangle seen from above one of its corners)
        and the integral of (e^{-beta r} - 1) cos / (4 pi r^2), which is O(beta)
        and only 1/r singular: Gauss-Legendre over the face's cells.  The outer
        integral over the voxel takes m_out points per dimension."""
        a, side = f >> 1, f & 1
        p, q = other_axes(a)
        plane = self.hi[a] if side else self.lo[a]
        P, w = self.nodes(v, m_out)
        z = np.abs(P[:, a] - plane)
        omega = np.zeros(len(P))
        for xp, sp_ in ((self.hi[p], 1.0), (self.lo[p], -1.0)):
            for xq, sq in ((self.hi[q], 1.0), (self.lo[q], -1.0)):
                dx, dy = xp - P[:, p], xq - P[:, q]
                omega += sp_ * sq * np.arctan2(dx * dy, z * np.sqrt(dx * dx + dy * dy + z * z))
        val = float(w @ omega) / (4.0 * np.pi)
        Pc, wc = self.nodes(v, m_corr)
        zc = np.abs(Pc[:, a] - plane)
        corr = 0.0
        for cq in range(self.n[q]):
            for cp in range(self.n[p]):
                Pj, wj = self.nodes(self.wall_index(f, cp, cq), m_corr)
                D = Pj[None, :, :] - Pc[:, None, :]
                r = np.sqrt(np.sum(D * D, axis=2))
                corr += float(wc @ (np.expm1(-beta * r) * (zc[:, None] / r) / (4.0 * np.pi * r * r)) @ wj)
        return (val + corr) / self.size(v)
