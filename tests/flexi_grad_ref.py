"""A float64 closed-form referee for the FlexiCubes gradient (k_flexi_bwd behind ops.flexicubes and engine.SdfObjective), CPU only.

Not autograd: every cube, patch and crossing edge (a, b) of the patch contributes, with D = s_b - s_a and g = gverts[v] / cnt
(v = the patch's dual vertex, cnt = the patch's number of crossing edges),

  to gs[a]   g . (x_a - x_b)  s_b / D^2          to gx[a]   g  s_b / D
  to gs[b]  -g . (x_a - x_b)  s_a / D^2          to gx[b]  -g  s_a / D

(u = (x_a s_b - x_b s_a) / D is the crossing point, the dual vertex the mean of its patch's crossings).  The terms are accumulated in
numpy in `dtype`; the scale arrays are the sums of the absolute values of the same terms, and errors are measured with
raster_grad_ref.measure:  err = max |got - ref| / max(scale, 1e-4 scale.max()).  1 / D^2 is taken as two divisions, (s / D) / D:
|s / D| <= 1 on a crossing edge, so the float32 evaluation overflows only where the value itself does.

Patch tables are oracle.flexi_ref.patch_tables(), vertex order is (cube, patch).  `corrupt` evaluates a deliberately wrong formula
(tests/test_flexi_grad.py's teeth).  The fields at the bottom are the inputs of that file."""
import functools

import numpy as np
import torch

from oracle import flexi_ref as FR
from raster_grad_ref import measure  # noqa: F401  (the one error measure of the gradient referees)

CORRUPTIONS = ("drop_patches", "cube_cnt", "swap_gs")
N_PATCH, EDGE_PATCH = FR.patch_tables()
MULTI_CODES = np.flatnonzero(N_PATCH > 1)
_CORNERS = np.array(FR.CORNERS)


def cube_codes(s, res):
    """Sign code of every cube ((res^3,), bit c = corner c inside, s < 0) from the SDF values as the extractor sees them."""
    G = res + 1
    inside = np.asarray(s).reshape(G, G, G) < 0
    code = np.zeros((res, res, res), np.int64)
    for c, (cx, cy, cz) in enumerate(FR.CORNERS):
        code |= inside[cx:cx + res, cy:cy + res, cz:cz + res].astype(np.int64) << c
    return code.reshape(-1)


def n_verts(s, res):
    return int(N_PATCH[cube_codes(s, res)].sum())


def grad(x, s, res, gverts, dtype=np.float64, corrupt=None):
    """x (G^3,3), s (G^3,), gverts (V,3) (numpy; s in the precision the extractor classifies it in) -> gs (G^3,), gx (G^3,3),
    scale_s, scale_x, all float64, evaluated in `dtype`."""
    assert corrupt is None or corrupt in CORRUPTIONS
    G = res + 1
    code = cube_codes(s, res)
    npc = N_PATCH[code].astype(np.int64)
    v_off = np.concatenate([[0], np.cumsum(npc)])
    assert len(gverts) == v_off[-1], (len(gverts), v_off[-1])
    x, s, gverts = (np.asarray(a).astype(dtype) for a in (x, s, gverts))
    x, s = x.reshape(-1, 3), s.reshape(-1)
    gs, gx, ss, sx = np.zeros(G ** 3, dtype), np.zeros((G ** 3, 3), dtype), np.zeros(G ** 3, dtype), np.zeros((G ** 3, 3), dtype)
    cubes = np.flatnonzero(npc > 0)
    ijk = np.stack(np.unravel_index(cubes, (res, res, res)), 1)
    corner = ((ijk[:, None, 0] + _CORNERS[None, :, 0]) * G + (ijk[:, None, 1] + _CORNERS[None, :, 1])) * G + (ijk[:, None, 2] + _CORNERS[None, :, 2])
    ep = EDGE_PATCH[code[cubes]]                                                 # (S,12)
    for p in range(1 if corrupt == "drop_patches" else 4):
        cnt = (ep >= 0).sum(1) if corrupt == "cube_cnt" else (ep == p).sum(1)
        for e, (a, b) in enumerate(FR.EDGES):
            sel = np.flatnonzero(ep[:, e] == p)
            if len(sel) == 0:
                continue
            ia, ib = corner[sel, a], corner[sel, b]
            g = gverts[v_off[cubes[sel]] + p] / cnt[sel, None].astype(dtype)
            sa, sb = s[ia], s[ib]
            D = sb - sa
            dot = (g * (x[ia] - x[ib])).sum(1)
            ta, tb = dot * ((sb / D) / D), -dot * ((sa / D) / D)
            if corrupt == "swap_gs":
                ta, tb = tb, ta
            wa, wb = g * (sb / D)[:, None], -g * (sa / D)[:, None]
            for acc, sc, idx, t in ((gs, ss, ia, ta), (gs, ss, ib, tb), (gx, sx, ia, wa), (gx, sx, ib, wb)):
                np.add.at(acc, idx, t)
                np.add.at(sc, idx, np.abs(t))
    return tuple(torch.from_numpy(a.astype(np.float64)) for a in (gs, gx, ss, sx))


def cotangent(n, seed=11):
    """Signed incoming vertex gradient (n,3), float32."""
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- fields: (x (G^3,3) float32, s (G^3,) float32, res)
def _jitter(x, res, extent, seed):
    """Every grid position moved by uniform +-0.3 of a cell (cell = extent / res): the grid stays unfolded, no two edges are parallel."""
    rng = np.random.default_rng(seed)
    return (x.double() + torch.from_numpy(rng.uniform(-0.3, 0.3, size=tuple(x.shape))) * (extent / res)).float()


FUZZ = tuple(f"fuzz{seed}" for seed in range(10))


def _fuzz(seed):
    """The field of test_flexi.py::test_hip_flexicubes_fuzz_random_fields(seed) -- same recipe, same seed -- on a jittered grid."""
    rng = np.random.default_rng(500 + seed)
    res = [6, 9, 12, 16][seed % 4]
    x = FR.construct_voxel_grid(res)[0] * 2.2
    k = rng.uniform(2.0, 9.0, size=(4, 3))
    ph = rng.uniform(0, 6.28, size=4)
    xt = x.numpy().astype(np.float64)
    s = sum(np.sin(xt @ k[i] + ph[i]) for i in range(4)) * 0.25 + rng.uniform(-0.3, 0.3)
    s = torch.from_numpy(s.astype(np.float32))
    s[torch.from_numpy(rng.random(len(s)) < 0.02)] = 0.0                       # exact zeros
    if seed % 2:
        s = torch.round(s * 4) / 4                                            # many ties and exact zeros
    return _jitter(x, res, 2.2, 900 + seed), s, res


ALLCASES_RES = 16


def allcases_code(a, b, c):
    return 1 + ((a * 8 + b) * 8 + c) % 254


def _allcases(seed=3):
    """res 16: cube (2a, 2b, 2c), a, b, c in 0..7, has sign code allcases_code(a, b, c); the designated cubes share no corner, so
    the codes hold by construction.  Magnitudes uniform in [0.05, 1]; the grid points of index 16 are +1."""
    res, G = ALLCASES_RES, ALLCASES_RES + 1
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.05, 1.0, size=(G, G, G))
    for a in range(8):
        for b in range(8):
            for c in range(8):
                code = allcases_code(a, b, c)
                for q, (cx, cy, cz) in enumerate(FR.CORNERS):
                    if (code >> q) & 1:
                        s[2 * a + cx, 2 * b + cy, 2 * c + cz] *= -1.0
    s[16, :, :] = s[:, 16, :] = s[:, :, 16] = 1.0
    x = FR.construct_voxel_grid(res)[0] * 2.2
    return _jitter(x, res, 2.2, 950), torch.from_numpy(s.reshape(-1).astype(np.float32)), res


def _tiny():
    """3^3 grid points, the centre at -1e-30, its six neighbours exactly 0 (outside), the rest +1: D = 1e-30 on the six crossing grid
    edges, D * D underflows in float32 while the gradient, up to 1e30 per unit of incoming gradient, fits."""
    res = 2
    s = torch.ones(3, 3, 3)
    for i, j, k in ((0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)):
        s[i, j, k] = 0.0
    s[1, 1, 1] = -1e-30
    x = FR.construct_voxel_grid(res)[0] * 2.2
    return _jitter(x, res, 2.2, 960), s.reshape(-1), res


CHAIN_RES = 14
CHAIN = ("chain_multi", "chain_multi_b")


@functools.lru_cache(maxsize=None)
def chain_scene(seed=0):
    """test_flexi.py's _chain_scene: the scene (torch and numpy forms), its grid and the mean radius of its object."""
    from helpers import make_scene
    sc = make_scene("ico2", 64, 64, seed=seed)
    x = FR.construct_voxel_grid(CHAIN_RES)[0] * 0.24
    r0 = float(sc["obj_verts"].norm(dim=1).mean())
    npsc = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}
    return sc, npsc, x, r0


def _chain_multi(variant):
    """The chain scene's grid (regular: SdfObjective shares one grid) and radius under a ripple of about one cell's wavelength: a closed
    surface with multi-patch cubes.  The second variant is the same ripple with another phase; it differs in vertex count."""
    _, _, x, r0 = chain_scene(0)
    xd = x.double()
    ph = (0.3, 1.0) if variant == 0 else (0.9, 1.0)
    s = xd.norm(dim=1) - r0 * (1.0 + 0.5 * torch.sin(120 * xd[:, 0] + ph[0]) * torch.cos(100.8 * xd[:, 1]) * torch.cos(108 * xd[:, 2] + ph[1]))
    return x, s.float(), CHAIN_RES


def _smooth(name):
    """The four smooth fields of test_flexi.py::test_hip_flexicubes_matches_oracle_index_for_index, at its resolutions."""
    res = 32 if name == "bumpy" else 24
    x = FR.construct_voxel_grid(res)[0] * 2.2
    r = x.norm(dim=1)
    s = {"sphere": lambda: r - 0.8,
         "torus": lambda: torch.stack([torch.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2) - 0.6, x[:, 2]], 1).norm(dim=1) - 0.25,
         "two_spheres": lambda: torch.minimum((x - 0.3).norm(dim=1) - 0.42, (x + 0.3).norm(dim=1) - 0.42),
         "bumpy": lambda: r - 0.7 + 0.08 * torch.sin(9 * x[:, 0]) * torch.cos(7 * x[:, 1]) * torch.sin(5 * x[:, 2])}[name]()
    return x, s, res


SMOOTH = ("sphere", "torus", "two_spheres", "bumpy")
FIELDS = FUZZ + ("allcases", "tiny") + CHAIN


@functools.lru_cache(maxsize=None)
def field(name):
    if name in FUZZ:
        return _fuzz(int(name[4:]))
    if name in CHAIN:
        return _chain_multi(CHAIN.index(name))
    if name in SMOOTH:
        return _smooth(name)
    return {"allcases": _allcases, "tiny": _tiny}[name]()


class Case:
    """A field, its cotangent and the float64 reference, computed once and shared by every test that names the field."""

    def __init__(self, name):
        self.name = name
        self.x, self.s, self.res = field(name)
        self.code = cube_codes(self.s.numpy(), self.res)
        self.nv = int(N_PATCH[self.code].sum())
        self.gv = cotangent(self.nv)
        self.ref = grad(self.x.numpy(), self.s.numpy(), self.res, self.gv.numpy())

    def n_multi(self):
        return int((N_PATCH[self.code] > 1).sum())


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
