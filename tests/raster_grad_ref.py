"""A float64 per-fragment referee for the rasteriser gradients (ops.raster_bwd, ops.raster_k_bwd, the facade), CPU only.

The arithmetic is oracle.ref_ops.eval_fragments' (perspective barycentrics with the w >= 0 clamp and the two floors, depth, the signed
squared distance to the nearest edge segment with the projection parameter held constant), restated here on an (n,3,3) LEAF that holds
every fragment's own copy of its face, so that autograd returns each fragment's own 3x3 gradient: the sum over fragments is the vertex
gradient, and the per-fragment magnitudes give the scale errors are measured against.  A face cut by the near plane goes through
pytorch3d's clip_faces restated in clip() below, and its sub-triangle barycentrics are mapped to the UNCLIPPED face's by face_bary(),
differentiably, crossing weights included -- the planes the forward operators return.

  err = max |got - ref| / max(scale, 1e-4 * scale.max())      scale (V,3) = sum over the fragments at the vertex of ||g_fragment||_inf

A fragment sits next to a kink of the function where (a) a perspective barycentric is near 0 (the w >= 0 mask, the inside sign) or
(b) the two smallest segment distances are nearly equal while their closest points differ (nearest-edge select).  `margin` measures
both; fragments under GUARD are taken out of a comparison on both sides by zeroing their incoming gradients (keep_mask)."""
import numpy as np
import torch

from oracle import ref_ops as R

K_EPS = R.K_EPS
GUARD = 1e-3
# every variant but None is deliberately wrong (tests/test_raster_grad.py's teeth): the barycentric gradient taken w.r.t. the
# sub-triangle, the crossing weights held constant, the area's derivative dropped, the w >= 0 mask of the
# clamp dropped, the inside sign of the distance dropped
VARIANTS = (None, "sub_bary", "detach_w", "no_area", "no_mask", "no_flip")


def _seg(px, py, ax, ay, bx, by):
    """ref_ops._seg_d2 and the segment's closest point (detached), for the tie exemption of the margin."""
    bax, bay = bx - ax, by - ay
    l2 = bax * bax + bay * bay
    deg = l2 <= K_EPS
    safe = torch.where(deg, torch.ones_like(l2), l2)
    t = ((bax * (px - ax) + bay * (py - ay)) / safe).clamp(0.0, 1.0).detach()      # envelope: t constant in the backward
    t = torch.where(deg, torch.ones_like(t), t)
    qx, qy = ax + t * bax, ay + t * bay
    dx, dy = qx - px, qy - py
    ex, ey = px - bx, py - by
    return torch.where(deg, ex * ex + ey * ey, dx * dx + dy * dy), torch.stack([qx, qy], 1).detach()


def evaluate(tri, xf, yf, variant=None):
    """tri (n,3,3) -> depth, clipped barycentrics (n,3), signed squared edge distance, decision margin."""
    x0, y0, z0 = tri[:, 0, 0], tri[:, 0, 1], tri[:, 0, 2]
    x1, y1, z1 = tri[:, 1, 0], tri[:, 1, 1], tri[:, 1, 2]
    x2, y2, z2 = tri[:, 2, 0], tri[:, 2, 1], tri[:, 2, 2]
    area = R._edge(x2, y2, x0, y0, x1, y1) + K_EPS
    if variant == "no_area":
        area = area.detach()
    a0 = R._edge(xf, yf, x1, y1, x2, y2) / area
    a1 = R._edge(xf, yf, x2, y2, x0, y0) / area
    a2 = R._edge(xf, yf, x0, y0, x1, y1) / area
    t0, t1, t2 = a0 * z1 * z2, z0 * a1 * z2, z0 * z1 * a2
    den = torch.clamp((t0 + t1) + t2, min=K_EPS)
    w = torch.stack([t0 / den, t1 / den, t2 / den], 1)
    cp = w.clamp(min=0.0)
    if variant == "no_mask":
        cp = w + (cp - w).detach()
    cb = cp / torch.clamp((cp[:, 0] + cp[:, 1]) + cp[:, 2], min=1e-5)[:, None]
    pz = (cb[:, 0] * z0 + cb[:, 1] * z1) + cb[:, 2] * z2
    (d01, q01), (d02, q02), (d12, q12) = _seg(xf, yf, x0, y0, x1, y1), _seg(xf, yf, x0, y0, x2, y2), _seg(xf, yf, x1, y1, x2, y2)
    ds = torch.stack([d01, d02, d12], 1)
    dist = torch.minimum(torch.minimum(d01, d02), d12)
    inside = (w > 0).all(1)
    sd = dist if variant == "no_flip" else torch.where(inside, -dist, dist)
    with torch.no_grad():
        order = ds.argsort(1)
        ar = torch.arange(len(ds))
        da, db = ds[ar, order[:, 0]], ds[ar, order[:, 1]]
        q = torch.stack([q01, q02, q12], 1)
        same = (q[ar, order[:, 0]] - q[ar, order[:, 1]]).abs().max(1).values <= 1e-9      # a shared vertex: either edge, same gradient
        m_edge = torch.where(same, torch.ones_like(da), (db - da) / db.clamp(min=1e-30))
        margin = torch.minimum(m_edge, w.abs().min(1).values)
    return pz, cb, sd, margin


def clip(fv, z_clip, variant=None):
    """pytorch3d clip_faces for rows of fv (n,3,3) that straddle z = z_clip (ref_ops.clip_subtriangles' operations, both halves at
    once).  Returns idx (n,3) = positions of (p1, p2, p3) in the face, nb (n,) = vertices behind, and per half (tri (n,3,3),
    m (n,3,3)): m's rows are the barycentrics of the half's vertices in (p1, p2, p3): p4 = (1 - w2, w2, 0), p5 = (1 - w3, 0, w3)."""
    c = torch.tensor(z_clip, dtype=torch.float32).to(fv.dtype)
    behind = fv[:, :, 2] < c
    nb = behind.sum(1)
    lone = torch.where((nb == 2)[:, None], ~behind, behind)
    i1 = lone.to(torch.int64).argmax(1)
    idx = torch.stack([i1, (i1 + 1) % 3, (i1 + 2) % 3], 1)
    ar = torch.arange(len(fv))
    p1, p2, p3 = fv[ar, idx[:, 0]], fv[ar, idx[:, 1]], fv[ar, idx[:, 2]]

    def crossing(po):
        w = (p1[:, 2] - c) / (p1[:, 2] - po[:, 2])
        u = 1.0 - w
        z = p1[:, 2] * u + po[:, 2] * w
        x = ((p1[:, 0] * p1[:, 2]) * u + (po[:, 0] * po[:, 2]) * w) / c
        y = ((p1[:, 1] * p1[:, 2]) * u + (po[:, 1] * po[:, 2]) * w) / c
        return w, torch.stack([x, y, z], 1)

    (w2, p4), (w3, p5) = crossing(p2), crossing(p3)
    if variant == "detach_w":
        w2, w3 = w2.detach(), w3.detach()
    z, o = torch.zeros_like(w2), torch.ones_like(w2)
    b4, b5 = torch.stack([1 - w2, w2, z], 1), torch.stack([1 - w3, z, w3], 1)
    e1, e2, e3 = torch.stack([o, z, z], 1), torch.stack([z, o, z], 1), torch.stack([z, z, o], 1)
    two = (nb == 2)[:, None, None]
    t0 = torch.where(two, torch.stack([p4, p5, p1], 1), torch.stack([p4, p2, p5], 1))
    m0 = torch.where(two, torch.stack([b4, b5, e1], 1), torch.stack([b4, e2, b5], 1))
    return idx, nb, (t0, m0), (torch.stack([p5, p2, p3], 1), torch.stack([b5, e2, e3], 1))


def face_bary(cb, m, idx):
    """Sub-triangle barycentrics -> the unclipped face's (pytorch3d convert_clipped_rasterization_to_original_faces):
    weights of (p1, p2, p3) = cb @ m, scattered to positions i1, i1 + 1, i1 + 2 (mod 3)."""
    r = (cb[:, :, None] * m).sum(1)
    return torch.zeros_like(r).scatter(1, idx, r)


class Referee:
    """Fragments of pix_to_face (H,W,K) on verts_ndc (V,3) / faces (F,3) (numpy, as oracle.clib.rasterize takes and returns them).
    The constructor evaluates every fragment in float64, chooses the half of a clipped face that reproduces the forward planes
    (clib.rasterize(K > 1) does not return it) and keeps the forward errors, the margins and the kept set; grad() differentiates."""

    def __init__(self, verts, faces, p2f, zbuf, bary, dists, z_clip):
        self.H, self.W, self.K = p2f.shape
        self.V, self.z_clip = len(verts), float(z_clip)
        self.verts, self.faces = torch.from_numpy(np.asarray(verts)), torch.from_numpy(np.asarray(faces, np.int64))
        flat = torch.from_numpy(np.ascontiguousarray(p2f)).reshape(-1)
        self.frag = (flat >= 0).nonzero(as_tuple=True)[0]                      # flat (pixel, k) index of every fragment
        self.fidx = self.faces[flat[self.frag]]                                 # (n,3) vertex ids
        zs = self.verts[self.fidx][:, :, 2]
        c32 = torch.tensor(self.z_clip, dtype=torch.float32)
        nb = (zs < c32).sum(1)
        self.strad = (nb == 1) | (nb == 2)
        self.second = None
        want = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).reshape((-1,) + d)[self.frag].double()
        Z, B, D = want(zbuf, ()), want(bary, (3,)), want(dists, ())
        with torch.no_grad():
            fv = self.verts.double()[self.fidx]
            pz, bf, sd, self.margin, (h0, h1) = self._forward(fv, None, both=True)
            # the half whose (z, signed distance) is the forward's; a fragment nearest to the edge the halves share has both equal
            # in the two (the forward then keeps the first half), and only its barycentrics tell which half it came from
            mis = lambda h: ((h[0] - Z).abs() / Z.abs().clamp(min=1e-30) + (h[2] - D).abs() / D.abs().clamp(min=1e-30)
                             + (h[1] - B).abs().max(1).values)
            self.second = self.strad & (nb == 1) & (mis(h1) < mis(h0))
            pz, bf, sd, self.margin, _ = self._forward(fv, None)
        self.fwd_err = dict(z=float((pz - Z).abs().max()), bary=float((bf - B).abs().max()),
                            dists=float(((sd - D).abs() / D.abs().clamp(min=1.0)).max()))      # absolute or relative
        self.keep = self.margin >= GUARD
        self.outside = D > 0

    def _coords(self, dt):
        pix = torch.div(self.frag, self.K, rounding_mode="floor")
        yi = torch.div(pix, self.W, rounding_mode="floor")
        xi = pix - yi * self.W
        return R.pix_ndc(self.W - 1 - xi, self.W, self.H, dt), R.pix_ndc(self.H - 1 - yi, self.H, self.W, dt)

    def _forward(self, fv, variant, both=False):
        xf, yf = self._coords(fv.dtype)
        pz, cb, sd, mg = evaluate(fv, xf, yf, variant)
        halves = None
        if bool(self.strad.any()):
            c = np.float32(self.z_clip).item()
            dummy = torch.tensor([[0.0, 0.0, 0.5 * c], [1.0, 0.0, 2.0 * c], [0.0, 1.0, 2.0 * c]], dtype=fv.dtype)
            fs = torch.where(self.strad[:, None, None], fv, dummy)              # the cut of a face that is not cut: never selected, kept finite
            idx, nb, (t0, m0), (t1, m1) = clip(fs, self.z_clip, variant)

            def half(t, m):
                hz, hc, hd, hm = evaluate(t, xf, yf, variant)
                return hz, (hc if variant == "sub_bary" else face_bary(hc, m, idx)), hd, hm

            h0, h1 = half(t0, m0), half(t1, m1)
            halves = (h0, h1)
            if not both:
                s, s2 = self.strad, self.second
                pick = lambda u, a, b: torch.where(s.reshape((-1,) + (1,) * (u.dim() - 1)),
                                                   torch.where(s2.reshape((-1,) + (1,) * (u.dim() - 1)), b, a), u)
                pz, cb, sd, mg = (pick(u, a, b) for u, a, b in zip((pz, cb, sd, mg), h0, h1))
        elif both:
            halves = ((pz, cb, sd, mg), (pz, cb, sd, mg))
        return pz, cb, sd, mg, halves

    def keep_mask(self):
        """(H,W,K) float32: 1 on fragments whose margin is at least GUARD, 0 on the others and on the background."""
        m = torch.zeros(self.H * self.W * self.K)
        m[self.frag[self.keep]] = 1.0
        return m.reshape(self.H, self.W, self.K)

    def planes(self, fv, variant=None):
        """(depth, face barycentrics, signed distance) of every fragment from per-fragment faces fv (n,3,3)."""
        return self._forward(fv, variant)[:3]

    def grad(self, gz=None, gb=None, gd=None, dtype=torch.float64, variant=None):
        """Incoming gradients (H,W,K) / (H,W,K,3) / (H,W,K) torch tensors or None -> (ref (V,3), scale (V,3), g (n,3,3)) in `dtype`
        arithmetic, returned as float64."""
        fv = self.verts.to(dtype)[self.fidx].clone().requires_grad_(True)
        pz, bf, sd = self.planes(fv, variant)
        loss = fv.sum() * 0
        if gz is not None:
            loss = loss + (pz * gz.reshape(-1)[self.frag].to(dtype)).sum()
        if gb is not None:
            loss = loss + (bf * gb.reshape(-1, 3)[self.frag].to(dtype)).sum()
        if gd is not None:
            loss = loss + (sd * gd.reshape(-1)[self.frag].to(dtype)).sum()
        g, = torch.autograd.grad(loss, fv)
        g = g.double()
        assert bool(torch.isfinite(g).all())
        rows = self.fidx.reshape(-1)
        ref = torch.zeros(self.V, 3, dtype=torch.float64).index_add_(0, rows, g.reshape(-1, 3))
        mag = g.abs().reshape(len(g), -1).max(1).values
        scale = torch.zeros(self.V, 3, dtype=torch.float64).index_add_(0, rows, mag[:, None, None].expand(-1, 3, 3).reshape(-1, 3))
        return ref, scale, g


def measure(got, ref, scale):
    """max |got - ref| / max(scale, 1e-4 scale.max()), and the position of the maximum."""
    e = (got.double().cpu() - ref).abs() / torch.clamp(scale, min=1e-4 * float(scale.max()))
    return float(e.max()), int(e.argmax())


# ---------------------------------------------------------------- scenes
def pruned_spheres(H, W):
    """rastk_ref.two_spheres without the faces whose smallest projected height (twice the area over the longest edge) is under one
    pixel, 2 / min(H, W) NDC: silhouette slivers, on which any float32 evaluation of the gradient is ill-conditioned."""
    import rastk_ref as RK
    v, f = RK.two_spheres(H, W)
    t = v[f].astype(np.float64)[:, :, :2]
    e = np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]], 1)
    area2 = np.abs(e[:, 0, 0] * e[:, 1, 1] - e[:, 0, 1] * e[:, 1, 0])
    height = area2 / np.sqrt((e ** 2).sum(-1)).max(1)
    return v, np.ascontiguousarray(f[height >= 2.0 / min(H, W)])


def six_clipped_faces(seed=7):
    """The two straddling faces of rastk_ref.near_plane() (one vertex behind the plane, two behind), each in all three cyclic vertex
    orders -- i1 = 0, 1, 2 -- scaled by 1 + 0.03 j and jittered by 2e-5 so that no two share a depth, and one plain face behind."""
    P3 = np.array([[[0.0, -0.0009, 0.002], [0.006, 0.004, 0.011], [-0.005, 0.005, 0.013]],
                   [[0.0, 0.0006, 0.012], [-0.004, -0.0015, 0.002], [0.004, -0.0012, 0.003]]], np.float64)
    rng = np.random.default_rng(seed)
    T = np.array([np.roll(P3[c], j, axis=0) * (1 + 0.03 * (2 * j + c)) + rng.normal(scale=2e-5, size=(3, 3))
                  for j in range(3) for c in range(2)])
    v = np.concatenate([T[..., :2] / T[..., 2:3], T[..., 2:3]], -1).reshape(-1, 3).astype(np.float32)
    far = np.array([[-0.9, -0.9, 0.5], [0.9, -0.9, 0.5], [0.0, 0.9, 0.5]], np.float32)
    v = np.concatenate([v, far])
    return v, np.arange(len(v), dtype=np.int64).reshape(-1, 3)
