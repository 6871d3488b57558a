"""Independent restatement of the gas box with one extinction coefficient per
voxel (include/rthx.h rthx_gasbox_trace_field) for the tests.

The library's ray crosses the lattice plane by plane and spends optical depth
in every cell.  This one never looks at a cell boundary: it is *delta
(Woodcock) tracking* -- tentative collisions at the field's largest beta, each
accepted with probability beta(x) / beta_max, the voxel found by locating the
collision point -- and a ray whose tentative path passes the uniform
restatement's wall distance (tests/gasbox_ref.py) ends at that wall.  The
rejected collisions make up exactly for the thinner voxels, so the absorption
law is the heterogeneous one although no segment is ever measured.

For a field that depends on z only the optical depth between two points is
closed form, which pins the restatement (and the device) to Gauss-Legendre
quadrature of the four kinds of exchange integral (pair_integral_layered).

Nothing here reads the library or shares code with it.
"""
from __future__ import annotations

import numpy as np

import gasbox_ref as G


class FieldBox(G.Box):
    """G.Box with beta[c_x, c_y, c_z] >= 0."""

    def __init__(self, lo, hi, n, beta):
        super().__init__(lo, hi, n)
        self.beta = np.asarray(beta, dtype=np.float64)
        assert self.beta.shape == tuple(self.n)

    def beta_elements(self):
        """The field in volume element order, c_x + n_x (c_y + n_y c_z)."""
        return np.array([self.beta[self.element(self.Ns + v)[2]] for v in range(self.Nv)])

    def cells(self, x):
        return np.clip(np.floor((x - self.lo) / self.h).astype(np.int64), 0, self.n - 1)

    def trace_row(self, g, R, rng):
        """Absorber counts [N] of R rays from emitter g."""
        kind, f, _c = self.element(g)
        lo_e, hi_e = self.bounds(g)
        o = lo_e + rng.random((R, 3)) * (hi_e - lo_e)
        phi = 2.0 * np.pi * rng.random(R)
        u = rng.random(R)
        d = np.empty((R, 3))
        if kind == "wall":
            a, side = f >> 1, f & 1
            p, q = G.other_axes(a)
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
        with np.errstate(divide="ignore", invalid="ignore"):
            t_ax = np.where(d == 0.0, np.inf, (np.where(d > 0.0, self.hi, self.lo) - o) / d)
        ax = np.argmin(t_ax, axis=1)
        t = t_ax[np.arange(R), ax]
        # walls first, for every ray; the rays absorbed in the gas are moved below
        end = self.cells(o + t[:, None] * d)
        face = 2 * ax + (d[np.arange(R), ax] > 0.0)
        cols = np.empty(R, dtype=np.int64)
        for a in range(3):
            p, q = G.other_axes(a)
            m = ax == a
            cols[m] = self.face_offset[face[m]] + end[m, p] + self.n[p] * end[m, q]
        bmax = float(self.beta.max())
        if bmax > 0.0:
            alive = np.arange(R)
            s = np.zeros(R)
            while alive.size:
                s[alive] += -np.log(1.0 - rng.random(alive.size)) / bmax
                alive = alive[s[alive] < t[alive]]  # (the rest reached their wall)
                c = self.cells(o[alive] + s[alive, None] * d[alive])
                hit = rng.random(alive.size) * bmax < self.beta[c[:, 0], c[:, 1], c[:, 2]]
                ch = c[hit]
                cols[alive[hit]] = self.Ns + ch[:, 0] + self.n[0] * (ch[:, 1] + self.n[1] * ch[:, 2])
                alive = alive[~hit]
        return np.bincount(cols, minlength=self.N)

    def trace(self, rows, R, seed):
        rng = np.random.default_rng(seed)
        return np.array([self.trace_row(int(g), R, rng) for g in rows])

    # -- quadrature for beta = beta(z) ------------------------------------------
    def pair_integral_layered(self, i, j, m=8):
        """F_ij by quadrature for a field that depends on z only: G.Box's four
        kernels with the optical depth tau between the points in place of
        beta r, and the absorber's own beta_j in place of beta.  With B the
        running integral of beta(z), tau = r (B(z2) - B(z1)) / (z2 - z1), and
        beta(z) r where z2 = z1."""
        bz = self.beta[0, 0, :]
        assert np.all(self.beta == bz[None, None, :])
        knots = self.lo[2] + self.h[2] * np.arange(self.n[2] + 1)
        Bk = np.concatenate([[0.0], np.cumsum(bz * self.h[2])])
        ki, fi, _ = self.element(i)
        kj, fj, cj = self.element(j)
        Pi, wi = self.nodes(i, m)
        Pj, wj = self.nodes(j, m)
        D = Pj[None, :, :] - Pi[:, None, :]
        r = np.sqrt(np.sum(D * D, axis=2))
        z1 = np.broadcast_to(Pi[:, None, 2], r.shape)
        z2 = np.broadcast_to(Pj[None, :, 2], r.shape)
        dz = z2 - z1
        level = dz == 0.0
        here = bz[np.clip(np.floor((z1 - self.lo[2]) / self.h[2]).astype(np.int64), 0, self.n[2] - 1)]
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(level, here, (np.interp(z2, knots, Bk) - np.interp(z1, knots, Bk)) / np.where(level, 1.0, dz))
        k = np.exp(-mean * r) / (r * r)
        if ki == "wall":
            k = k * np.maximum(0.0, D @ self.inward_normal(fi)) / r / np.pi
        else:
            k = k / (4.0 * np.pi)
        if kj == "wall":
            k = k * np.maximum(0.0, -(D @ self.inward_normal(fj))) / r
        else:
            k = k * bz[cj[2]]
        return float(wi @ k @ wj) / self.size(i)


# -- cases shared by the CPU and the GPU tests ------------------------------------
LAYERS = (0.5, 3.0, 1.0)


def layered_box():
    return FieldBox([0, 0, 0], [1, 1, 1], (3, 3, 3), np.broadcast_to(np.array(LAYERS), (3, 3, 3)))


def layered_rows(box):
    return [box.volume_index(0, 0, 0), box.wall_index(4, 0, 0), box.wall_index(0, 1, 1)]


def check_rows_against_layered_quadrature(box, rows, counts, R):
    """Every column at least one cell away from its emitter within 5 sigma
    (binomial) of the layered quadrature; returns (worst |z|, pairs)."""
    kinds, worst, pairs = set(), 0.0, 0
    for k, i in enumerate(rows):
        assert counts[k].sum() == R
        for j in range(box.N):
            if not box.separated(i, j):
                continue
            q = box.pair_integral_layered(i, j)
            if q == 0.0:  # (coplanar wall cells never see each other)
                assert counts[k, j] == 0, (i, j)
                continue
            z = (counts[k, j] / R - q) / np.sqrt(q * (1.0 - q) / R)
            worst = max(worst, abs(z))
            pairs += 1
            kinds.add((box.element(i)[0], box.element(j)[0]))
            assert abs(z) <= 5.0, (i, j, counts[k, j] / R, q, z)
    assert kinds == {("vol", "vol"), ("vol", "wall"), ("wall", "vol"), ("wall", "wall")}
    return worst, pairs


THIN_SCALE = 1e-3


def thin_field():
    """kappa_v = 1e-3 (0.5, 1, 2)[(c_x + c_y + c_z) mod 3] on the 3 x 3 x 3 lattice."""
    cx, cy, cz = np.meshgrid(range(3), range(3), range(3), indexing="ij")
    return THIN_SCALE * np.array([0.5, 1.0, 2.0])[(cx + cy + cz) % 3]


def thin_reference(ref, R):
    """(T_g / T)^4 of every voxel of the unit cube with the z- face hot, the
    rest cold and black, and a gas so thin that it exchanges with the walls
    alone: F(voxel -> z- face) by quadrature, and the tolerance 5 sigma
    (binomial at R) + 2e-3.  The factor is geometric to first order; it is
    taken at the field's mean kappa, which is within 1e-3 of every voxel's
    own, so the attenuation left out or put in too much is below 1e-3 * sqrt(3)
    * F < 6e-4, inside the 2e-3."""
    kbar = float(thin_field().mean())
    q = np.array([ref.volume_to_face(ref.Ns + v, 4, kbar) for v in range(ref.Nv)])
    return q, 5.0 * np.sqrt(q * (1.0 - q) / R) + 2e-3
