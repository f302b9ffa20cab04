"""Sparse FlexiCubes (followmyhold_amd/sparse_flexi.py, libfoho_sflexi.so): the mesh of ops.flexicubes from the field and three per-axis
coordinate tables.  The yardstick everywhere is the dense extractor (itself tested against oracle/flexi_ref.py) and every comparison is
torch.equal: vertices, faces and l_dev, in the same order.  CPU: the library, its exports, argument validation, the workspace bound,
grid_axes against generate_dense_grid_points, the pipeline switch's validation.  GPU: analytic and random fields, boundary and
single-point cases, capacities through ctypes, streams, and the pipeline switch."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from followmyhold_amd import _lib, ops, pipeline as PLN, sparse_flexi as SF, standins  # noqa: E402
from followmyhold_amd.facade import generate_dense_grid_points  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "followmyhold_amd", "csrc")
BMIN, BMAX = np.array([-1.0, -0.8, -1.2]), np.array([1.1, 0.9, 0.7])      # different bounds per axis
vp = ctypes.c_void_p


def _make():
    subprocess.check_call(["make", "-C", CSRC, "-s"])


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = sorted(l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3 and l.split()[-2] in ("T", "t", "W", "V", "B", "D"))
    return [n for n in names if not n.startswith(("_init", "_fini", "__bss_start", "_edata", "_end", "__hip_"))]


# ---------------------------------------------------------------- CPU
def test_sflexi_library_builds_and_exports_exactly_its_header():
    _make()
    assert os.path.exists(SF.SO_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "foho_sflexi.h")).read(), flags=re.S)
    want = sorted(set(re.findall(r"\b(foho_sflexi_\w+)\s*\(", src)))
    assert "foho_sflexi_version" in want and "foho_sflexi_last_error" in want and "foho_sflexi_extract" in want, want
    assert _exported(SF.SO_PATH) == want


def test_binding_validates_arguments_without_a_gpu():
    _make()
    L = SF.lib()
    assert L.foho_sflexi_version() == SF.VERSION
    one = vp(256)                  # a non-null pointer that is never dereferenced: every call below is refused before any launch
    big = ctypes.c_size_t(1 << 40)

    def refused(status, *words):
        msg = L.foho_sflexi_last_error().decode()
        assert status < 0 and all(w in msg for w in words), (status, msg)

    refused(L.foho_sflexi_mark(None, 8, one, big, one, None), "foho_sflexi_mark", "null")
    refused(L.foho_sflexi_mark(one, 8, None, big, one, None), "foho_sflexi_mark", "null")
    refused(L.foho_sflexi_mark(one, 8, one, big, None, None), "foho_sflexi_mark", "null")
    for res in (0, 1025, -3):
        refused(L.foho_sflexi_mark(one, res, one, big, one, None), "foho_sflexi_mark", "resolution")
        assert L.foho_sflexi_mark_bytes(res) == 0 and L.foho_sflexi_workspace_bytes(res, 10) == 0
    refused(L.foho_sflexi_mark(one, 8, one, L.foho_sflexi_mark_bytes(8) - 1, one, None), "foho_sflexi_mark", "too small")

    def extract(axes=one, s=one, res=8, marks=one, mb=big, cap=10, verts=one, vc=40, faces=one, fc=60, ldev=one, counts=one, ws=one, wb=big):
        return L.foho_sflexi_extract(axes, s, res, marks, mb, cap, verts, vc, faces, fc, ldev, counts, ws, wb, None)

    for name in ("axes", "s", "marks", "verts", "faces", "counts", "ws"):
        refused(extract(**{name: None}), "foho_sflexi_extract", "null")
    for res in (0, 1025):
        refused(extract(res=res), "foho_sflexi_extract", "resolution")
    for kw in (dict(cap=-1), dict(cap=SF.MAX_CUBES + 1), dict(vc=-1), dict(fc=-1)):
        refused(extract(**kw), "foho_sflexi_extract", "capacity")
    refused(extract(mb=L.foho_sflexi_mark_bytes(8) - 1), "foho_sflexi_extract", "too small")
    refused(extract(wb=L.foho_sflexi_cube_bytes(10) - 1), "foho_sflexi_extract", "too small")
    assert L.foho_sflexi_cube_bytes(-1) == 0 and L.foho_sflexi_cube_bytes(SF.MAX_CUBES + 1) == 0


def test_workspace_is_monotone_and_a_tenth_of_the_dense_one():
    _make()
    L, H = SF.lib(), _lib.lib()
    sizes = [L.foho_sflexi_workspace_bytes(384, c) for c in (0, 1, 1000, 100_000, 2_000_000, 20_000_000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert L.foho_sflexi_workspace_bytes(384, 2_000_000) <= H.foho_flexi_workspace_bytes(384) // 10
    assert L.foho_sflexi_workspace_bytes(384, 2_000_000) == L.foho_sflexi_mark_bytes(384) + L.foho_sflexi_cube_bytes(2_000_000)
    assert (L.foho_sflexi_cube_bytes(2_000_000) - L.foho_sflexi_cube_bytes(1_000_000)) / 1_000_000 < 40      # bytes per surface cube
    assert L.foho_sflexi_workspace_bytes(1024, 1000) > 0 and L.foho_sflexi_workspace_bytes(1, 0) > 0


@pytest.mark.parametrize("res", [8, 13])
def test_grid_axes_mesh_to_the_dense_grid(res):
    ax = SF.grid_axes(BMIN, BMAX, res)
    assert ax.shape == (3, res + 1) and ax.dtype == torch.float32
    xyz, _, _ = generate_dense_grid_points(BMIN, BMAX, octree_depth=5, octree_resolution=res, indexing="ij")
    xs, ys, zs = np.meshgrid(*ax.numpy(), indexing="ij")
    assert np.array_equal(np.stack((xs, ys, zs), axis=-1).reshape(-1, 3), xyz)
    assert not np.array_equal(ax.numpy(), ax.half().float().numpy())       # not the fp16-rounded tables of volume.axis_tables


def test_final_extract_switch_is_validated(monkeypatch):
    assert PLN.final_extract_mode() == "dense" and PLN.final_extract_mode("sparse") == "sparse"
    with pytest.raises(_lib.FohoError):
        PLN.final_extract_mode("nonsense")
    monkeypatch.setenv("FOHO_FINAL_EXTRACT", "sparse")
    assert PLN.final_extract_mode() == "sparse" and PLN.final_extract_mode("dense") == "dense"      # the kwarg overrides the environment
    monkeypatch.setenv("FOHO_FINAL_EXTRACT", "nonsense")
    assert PLN.final_extract_mode("sparse") == "sparse"
    with pytest.raises(_lib.FohoError, match="nonsense"):
        PLN.final_extract_mode()
    pipe = standins.make_standin_pipeline(device="cpu", dtype=torch.float32, seed=1)

    def no_work(*a, **k):
        raise AssertionError("a network ran before the switch was validated")

    monkeypatch.setattr(pipe, "prepare_image", no_work)
    monkeypatch.setattr(pipe, "encode_cond", no_work)
    with pytest.raises(_lib.FohoError, match="nonsense"):          # from the environment
        pipe(image=None, final_octree_resolution=32)
    with pytest.raises(_lib.FohoError, match="nonsense"):
        pipe.call_batch([None], [{}], final_octree_resolution=32)
    monkeypatch.delenv("FOHO_FINAL_EXTRACT")
    with pytest.raises(_lib.FohoError, match="nonsense"):          # from the argument
        pipe(image=None, final_octree_resolution=32, final_extract="nonsense")
    with pytest.raises(_lib.FohoError, match="nonsense"):
        pipe.call_batch([None], [{}], final_octree_resolution=32, final_extract="nonsense")


# ---------------------------------------------------------------- GPU
def _grid(res):
    xyz, _, _ = generate_dense_grid_points(BMIN, BMAX, octree_depth=5, octree_resolution=res, indexing="ij")
    return torch.as_tensor(xyz, dtype=torch.float32, device="cuda")


def _shape(name, x):
    """Fields that are negative inside, on the grid points x (N, 3)."""
    c = torch.tensor([0.05, 0.05, -0.25], device=x.device)
    p = x - c
    if name == "sphere":
        return p.norm(dim=1) - 0.6
    if name == "torus":
        q = torch.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - 0.45
        return torch.sqrt(q * q + p[:, 2] ** 2) - 0.2
    if name == "blobs":
        a = (x - torch.tensor([-0.45, 0.0, -0.3], device=x.device)).norm(dim=1) - 0.3
        b = (x - torch.tensor([0.5, 0.2, -0.1], device=x.device)).norm(dim=1) - 0.25
        return torch.minimum(a, b)
    if name == "crossing":         # a ball larger than the box: the surface leaves through all six sides
        return (x - torch.tensor([0.05, 0.05, -0.25], device=x.device)).norm(dim=1) - 1.0
    raise KeyError(name)


def _codes(s, res):
    """Corner code of every cube (x-fastest corner order, inside = s < 0), numpy (res, res, res)."""
    b = (s.reshape(res + 1, res + 1, res + 1) < 0).astype(np.int64)
    c = np.zeros((res, res, res), np.int64)
    for q in range(8):
        c |= b[(q & 1):(q & 1) + res, ((q >> 1) & 1):((q >> 1) & 1) + res, (q >> 2):(q >> 2) + res] << q
    return c


# signs of a 9^3 field whose 512 cubes show all 256 corner codes: an i.i.d. draw, then single signs flipped until every code occurs
# (512 i.i.d. cubes alone miss about 35 codes)
_SIGNS8 = ("91335a66406fe2de445edeb300c2b02e724f1e5012280a9ffd2b8ab62d666d042ed06e068a705b35d003d8876eea5b9bfd7f9032b131cd4c99d48d3e945c"
           "b3d06f66aba551545842e00bdcf15cd9ee0f2f4f68cb9d9a85b7f8129380")


def _random_field(res):
    if res == 8:
        neg = np.unpackbits(np.frombuffer(bytes.fromhex(_SIGNS8), np.uint8))[:729].astype(bool)
        mag = np.abs(np.random.default_rng(8).standard_normal(729).astype(np.float32)) + np.float32(1e-3)
        return np.where(neg, -mag, mag).astype(np.float32)
    return np.random.default_rng(0).standard_normal((res + 1,) * 3).astype(np.float32).reshape(-1)


def _same(res, s, x=None, want_nonempty=True):
    """flexicubes_sparse against ops.flexicubes on the dense grid: vertices, faces, l_dev bit for bit; -> the stats."""
    x = _grid(res) if x is None else x
    v0, f0, l0 = ops.flexicubes(x, s, res)
    v1, f1, l1, st = SF.flexicubes_sparse(SF.grid_axes(BMIN, BMAX, res), s, res, return_stats=True)
    assert v1.dtype == v0.dtype and f1.dtype == torch.int64 and l1.dtype == l0.dtype
    assert v1.shape == v0.shape and f1.shape == f0.shape and l1.shape == l0.shape, (v0.shape, v1.shape, f0.shape, f1.shape)
    assert torch.equal(v0, v1) and torch.equal(f0, f1) and torch.equal(l0, l1)
    assert st["vertices"] == v0.shape[0] and st["faces"] == f0.shape[0]
    if want_nonempty:
        assert v0.shape[0] > 0 and f0.shape[0] > 0
    return st


@gpu
@pytest.mark.parametrize("res", [33, 64])
@pytest.mark.parametrize("name", ["sphere", "torus", "blobs"])
def test_analytic_fields_give_the_dense_mesh(name, res):
    x = _grid(res)
    s = _shape(name, x)
    st = _same(res, s, x)
    codes = _codes(s.cpu().numpy(), res)
    assert st["cubes"] == int(((codes != 0) & (codes != 255)).sum())
    assert st["workspace_bytes"] == SF.lib().foho_sflexi_workspace_bytes(res, st["cubes"])


@gpu
@pytest.mark.parametrize("res", [8, 13])
def test_random_signs_cover_every_case(res):
    """Every row of the patch tables, the ambiguous cases included; 13^3 = 2197 cubes leave the last mask word partial."""
    s = _random_field(res)
    assert len(np.unique(_codes(s, res))) == 256
    _same(res, torch.from_numpy(s).cuda())


@gpu
@pytest.mark.parametrize("res", [13, 32])
def test_surface_crossing_the_boundary_on_all_six_sides(res):
    x = _grid(res)
    s = _shape("crossing", x)
    codes = _codes(s.cpu().numpy(), res)
    mixed = (codes != 0) & (codes != 255)
    for side in (mixed[0], mixed[-1], mixed[:, 0], mixed[:, -1], mixed[:, :, 0], mixed[:, :, -1]):
        assert side.any()                    # surface cubes at index 0 and res-1 of every axis: their outer edges own no quad
    _same(res, s, x)


@gpu
def test_exact_zeros_on_the_surface_are_outside():
    res = 16
    G = res + 1
    i, j, k = torch.meshgrid(*[torch.arange(G, device="cuda", dtype=torch.float32)] * 3, indexing="ij")
    s = (torch.maximum(torch.maximum((i - 8).abs(), (j - 8).abs()), (k - 7).abs()) - 3.0).reshape(-1)       # a box with faces ON grid planes
    assert int((s == 0).sum()) > 100 and int((s < 0).sum()) == 125
    _same(res, s)
    s2 = _shape("sphere", _grid(res))
    s2[s2.abs() < 0.05] = 0.0                # zeros on both sides of a curved surface
    assert int((s2 == 0).sum()) > 50
    _same(res, s2)


@gpu
@pytest.mark.parametrize("res,point", [(12, (5, 6, 7)), (12, (1, 10, 8)), (12, (2, 10, 4)), (12, (1, 1, 1)), (12, (11, 11, 11)), (12, (0, 0, 0)), (12, (12, 12, 12)),
                                       (13, (12, 12, 12))])
def test_single_negative_grid_point(res, point):
    """One inside point: 8 surface cubes in the interior ((5,6,7)); (1,10,8) at res 12 puts the neighbouring cubes 127 and 128 on either
    side of a 64-cube word boundary, (2,10,4) the cubes 255 and 256 on either side of a 256-cube block of the rank prefix; (1,1,1) and
    (res-1,..) include cube ids 0 and res^3-1; the grid's own corners give ONE surface cube (id 0, id res^3-1) and no face."""
    G = res + 1
    s = torch.ones(G, G, G, device="cuda")
    s[point] = -0.7
    corner = all(p in (0, res) for p in point)
    st = _same(res, s.reshape(-1) * 0.3, want_nonempty=not corner)
    assert st["cubes"] == (1 if corner else 8)
    ids = sorted(((point[0] - a) * res + (point[1] - b)) * res + (point[2] - c) for a in (0, 1) for b in (0, 1) for c in (0, 1)
                 if all(0 <= p - d < res for p, d in zip(point, (a, b, c))))
    if point == (1, 10, 8):
        assert 127 in ids and 128 in ids
    if point == (2, 10, 4):
        assert 255 in ids and 256 in ids
    if point == (1, 1, 1):
        assert ids[0] == 0
    if point == (11, 11, 11) or point[0] == res:
        assert ids[-1] == res ** 3 - 1
    if not corner:
        assert st["vertices"] == 8 and st["faces"] == 12


@gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_one_sign_fields_are_empty(sign):
    res = 20
    s = torch.full(((res + 1) ** 3,), 0.25 * sign, device="cuda")
    v, f, l, st = SF.flexicubes_sparse(SF.grid_axes(BMIN, BMAX, res), s, res, return_stats=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and l.shape == (0,) and f.dtype == torch.int64
    assert st["cubes"] == 0 and st["vertices"] == 0 and st["faces"] == 0
    _same(res, s, want_nonempty=False)


@gpu
def test_torus_at_128():
    x = _grid(128)
    st = _same(128, _shape("torus", x), x)
    assert st["cubes"] > 20000


@gpu
def test_repeatable_and_stream_independent():
    res = 48
    x = _grid(res)
    s = _shape("blobs", x)
    ax = SF.grid_axes(BMIN, BMAX, res).cuda()
    a = SF.flexicubes_sparse(ax, s, res)
    b = SF.flexicubes_sparse(ax, s, res)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = SF.flexicubes_sparse(ax, s, res)
    side.synchronize()
    for other in (b, c):
        assert all(torch.equal(p, q) for p, q in zip(a, other))
    assert a[0].shape[0] > 1000


def _sparse_raw(ax, s, res, n_cubes, verts_cap, faces_cap, guard, want_ldev=True):
    """foho_sflexi_mark + _extract through ctypes into buffers with `guard` extra elements of a known pattern behind each capacity;
    want_ldev False: a null l_dev (the buffer comes back untouched)."""
    L = SF.lib()
    st = vp(torch.cuda.current_stream().cuda_stream)
    nm = L.foho_sflexi_mark_bytes(res)
    marks = torch.empty(nm, dtype=torch.uint8, device="cuda")
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.foho_sflexi_mark(vp(s.data_ptr()), res, vp(marks.data_ptr()), nm, vp(n_dev.data_ptr()), st) == 0
    assert int(n_dev.item()) == n_cubes
    nw = L.foho_sflexi_cube_bytes(n_cubes)
    ws = torch.empty(nw, dtype=torch.uint8, device="cuda")
    verts = torch.full((verts_cap * 3 + guard,), -7.5, device="cuda")
    faces = torch.full((faces_cap * 3 + guard,), -77, dtype=torch.int64, device="cuda")
    ldev = torch.full((verts_cap + guard,), -7.5, device="cuda")
    counts = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    assert L.foho_sflexi_extract(vp(ax.data_ptr()), vp(s.data_ptr()), res, vp(marks.data_ptr()), nm, n_cubes, vp(verts.data_ptr()), verts_cap,
                                 vp(faces.data_ptr()), faces_cap, vp(ldev.data_ptr()) if want_ldev else None, vp(counts.data_ptr()), vp(ws.data_ptr()), nw,
                                 st) == 0
    return verts, faces, ldev, counts.tolist()


def _dense_raw(x, s, res, verts_cap, faces_cap, guard, want_ldev=True):
    H = _lib.lib()
    nws = H.foho_flexi_workspace_bytes(res)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    verts = torch.full((verts_cap * 3 + guard,), -7.5, device="cuda")
    faces = torch.full((faces_cap * 3 + guard,), -77, dtype=torch.int64, device="cuda")
    ldev = torch.full((verts_cap + guard,), -7.5, device="cuda")
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    _lib.check(H.foho_flexi_fwd(vp(x.data_ptr()), vp(s.data_ptr()), res, vp(verts.data_ptr()), verts_cap, vp(faces.data_ptr()), faces_cap,
                                vp(ldev.data_ptr()) if want_ldev else None, vp(counts.data_ptr()), vp(ws.data_ptr()), ctypes.c_size_t(nws),
                                vp(torch.cuda.current_stream().cuda_stream)), "foho_flexi_fwd")
    return verts, faces, ldev, counts.tolist()


@gpu
@pytest.mark.parametrize("want_ldev", [True, False])
def test_all_codes_field_equals_dense_with_and_without_l_dev(want_ldev):
    """Both extractors call one per-cube core (csrc/flexi_core.h); on the 9^3 field that shows all 256 corner codes they agree bit for bit
    with l_dev requested and with a null l_dev, and a null l_dev leaves nothing written."""
    res, guard = 8, 8
    s = torch.from_numpy(_random_field(res)).cuda()
    codes = _codes(s.cpu().numpy(), res)
    n = int(((codes != 0) & (codes != 255)).sum())
    vc, fc = 4 * n, 6 * n                  # at most 4 vertices and 6 triangles per surface cube
    sv, sf_, sl, sc = _sparse_raw(SF.grid_axes(BMIN, BMAX, res).cuda(), s, res, n, vc, fc, guard, want_ldev)
    dv, df, dl, dc = _dense_raw(_grid(res), s, res, vc, fc, guard, want_ldev)
    nv, nf, over = sc
    assert sc == dc and over == 0 and nv > n and nf > 0, (sc, dc)
    assert torch.equal(sv[:nv * 3], dv[:nv * 3]) and torch.equal(sf_[:nf * 3], df[:nf * 3])
    if want_ldev:
        assert torch.equal(sl[:nv], dl[:nv]) and bool((sl[:nv] >= 0).all())
    else:
        assert bool((sl == -7.5).all()) and bool((dl == -7.5).all())


@gpu
def test_small_capacities_set_the_dense_overflow_bits_and_write_nothing_past_them():
    res, guard = 24, 64
    x = _grid(res)
    s = _shape("sphere", x).contiguous()
    ax = SF.grid_axes(BMIN, BMAX, res).cuda()
    v_full, f_full, _, st = SF.flexicubes_sparse(ax, s, res, return_stats=True)
    nv, nf, n = st["vertices"], st["faces"], st["cubes"]
    assert nv > 500 and nf > 1000
    for vc, fc, bits in [(nv, nf, 0), (nv - 1, nf, 1), (nv, nf - 1, 2), (nv // 2, nf // 3, 3), (1, 1, 3), (nv + 5, nf + 7, 0)]:
        sv, sf_, sl, sc = _sparse_raw(ax, s, res, n, vc, fc, guard)
        dv, df, dl, dc = _dense_raw(x, s, res, vc, fc, guard)
        assert sc == dc == [nv, nf, bits], (vc, fc, sc, dc)
        assert torch.equal(sv[vc * 3:], torch.full((guard,), -7.5, device="cuda")) and torch.equal(sl[vc:], torch.full((guard,), -7.5, device="cuda"))
        assert torch.equal(sf_[fc * 3:], torch.full((guard,), -77, dtype=torch.int64, device="cuda"))
        if bits == 0:
            assert torch.equal(sv[:nv * 3], v_full.reshape(-1)) and torch.equal(sf_[:nf * 3], f_full.reshape(-1))
            assert torch.equal(sv[:nv * 3], dv[:nv * 3]) and torch.equal(sf_[:nf * 3], df[:nf * 3]) and torch.equal(sl[:nv], dl[:nv])
    # fewer cube slots than surface cubes: refused as a whole, nothing extracted
    L = SF.lib()
    stp = vp(torch.cuda.current_stream().cuda_stream)
    nm = L.foho_sflexi_mark_bytes(res)
    marks = torch.empty(nm, dtype=torch.uint8, device="cuda")
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.foho_sflexi_mark(vp(s.data_ptr()), res, vp(marks.data_ptr()), nm, vp(n_dev.data_ptr()), stp) == 0
    cap = n - 1
    nw = L.foho_sflexi_cube_bytes(cap)
    ws = torch.empty(nw, dtype=torch.uint8, device="cuda")
    verts = torch.full((nv * 3,), -7.5, device="cuda")
    faces = torch.full((nf * 3,), -77, dtype=torch.int64, device="cuda")
    counts = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    assert L.foho_sflexi_extract(vp(ax.data_ptr()), vp(s.data_ptr()), res, vp(marks.data_ptr()), nm, cap, vp(verts.data_ptr()), nv,
                                 vp(faces.data_ptr()), nf, None, vp(counts.data_ptr()), vp(ws.data_ptr()), nw, stp) == 0
    assert counts.tolist() == [0, 0, SF.OVER_CUBES]
    assert bool((verts == -7.5).all()) and bool((faces == -77).all())


@gpu
def test_a_field_that_requires_grad_is_refused():
    res = 8
    s = _shape("sphere", _grid(res)).requires_grad_(True)
    with pytest.raises(_lib.FohoError, match="forward only"):
        SF.flexicubes_sparse(SF.grid_axes(BMIN, BMAX, res), s, res)
    with pytest.raises(_lib.FohoError, match="forward only"):
        ops.flexicubes_sparse(SF.grid_axes(BMIN, BMAX, res), s, res)


# ---------------------------------------------------------------- the pipeline switch
def _pipeline_setup(tmp_path):
    from PIL import Image
    from followmyhold_amd import geo_decode
    from test_pipeline import _renderer, _scene_for_pipeline, _short_config, _write
    sc = _scene_for_pipeline()
    paths = _write(tmp_path, sc)
    img = Image.open(paths["cropped_obj_img_path"])
    # Two whole runs are bitwise repeatable only without optimisation iterations: the step's backward accumulates with float atomics
    # (DESIGN.md section 11).  So the runs compared bit for bit across calls keep the schedule, the networks and the seeds of
    # tests/test_volume_decode.py's pipeline test and take no inner iterations; the run WITH iterations is checked inside the run, where
    # the sparse extraction is compared with the dense extraction of the very same field.
    cfg = _short_config()
    cfg.optimization_steps_hand = cfg.optimization_steps_scale = cfg.optimization_steps_joint = 0
    pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1, num_latents=128, embed_dim=8, width=128, heads=2,
                                          layers=1, num_freqs=8)
    geo_decode.install(pipe.vae)
    kw = dict(config=cfg, renderer=_renderer(sc["fov"]), J_regressor=sc["J_regressor"], guidance_octree_resolution=16, final_octree_resolution=32)
    return pipe, img, paths, kw, _short_config


class _GridCalls:
    def __init__(self, monkeypatch):
        self.res = []
        orig = PLN.generate_dense_grid_points

        def counted(bmin, bmax, octree_depth, indexing="ij", octree_resolution=None):
            self.res.append(int(octree_resolution))
            return orig(bmin, bmax, octree_depth, indexing=indexing, octree_resolution=octree_resolution)

        monkeypatch.setattr(PLN, "generate_dense_grid_points", counted)


def _mesh_equal(a, b):
    (o1, h1), (o2, h2) = a, b
    assert o1.verts_packed().shape[0] > 100
    assert torch.equal(o1.verts_packed(), o2.verts_packed()) and torch.equal(o1.faces_packed(), o2.faces_packed())
    assert torch.equal(h1.verts_packed(), h2.verts_packed()) and torch.equal(h1.faces_packed(), h2.faces_packed())


@gpu
def test_pipeline_final_extract_switch(tmp_path, monkeypatch):
    pipe, img, paths, kw, short_config = _pipeline_setup(tmp_path)
    grids = _GridCalls(monkeypatch)

    def run(**extra):
        grids.res.clear()
        out = pipe(image=[img], mc_algo="mc", generator=torch.manual_seed(2), sil_renderer=None, **{**kw, **extra}, **paths)
        return out, list(grids.res), dict(pipe.stats)

    base, g, st = run()
    assert g.count(32) == 1 and "final_extract" not in st
    for decode in ("dense", "hierarchical"):
        ref, g, st = run(final_decode=decode)
        assert g.count(32) == 1 and "final_extract" not in st          # the default route builds the final point grid once
        got, g, st = run(final_decode=decode, final_extract="sparse")
        _mesh_equal(ref, got)
        assert g.count(32) == (0 if decode == "hierarchical" else 1)     # hierarchical + sparse: never built
        fe = st["final_extract"]
        assert fe["vertices"] == got[0].verts_packed().shape[0] and fe["faces"] == got[0].faces_packed().shape[0]
        assert fe["cubes"] > 0 and fe["workspace_bytes"] == SF.lib().foho_sflexi_workspace_bytes(32, fe["cubes"])
    _mesh_equal(base, run(final_decode="dense")[0])
    monkeypatch.setenv("FOHO_FINAL_EXTRACT", "sparse")
    got, g, st = run(final_decode="hierarchical")
    _mesh_equal(base, got)
    assert g.count(32) == 0 and "final_extract" in st
    got, g, st = run(final_decode="hierarchical", final_extract="dense")           # the kwarg overrides the environment
    assert g.count(32) == 1 and "final_extract" not in st
    monkeypatch.delenv("FOHO_FINAL_EXTRACT")

    # with optimisation iterations: the sparse mesh equals the dense extraction of the same field, inside the run
    checked = []
    orig = ops.flexicubes_sparse

    def spy(axes, s, res, return_stats=False):
        out = orig(axes, s, res, return_stats=return_stats)
        xyz, _, _ = generate_dense_grid_points(np.full(3, -1.10), np.full(3, 1.10), octree_depth=5, octree_resolution=res, indexing="ij")
        v0, f0, l0 = ops.flexicubes(torch.as_tensor(xyz, dtype=torch.float32, device=s.device), s, res)
        checked.append(res)
        assert v0.shape[0] > 100 and torch.equal(v0, out[0]) and torch.equal(f0, out[1]) and torch.equal(l0, out[2])
        return out

    monkeypatch.setattr(ops, "flexicubes_sparse", spy)
    cfg = short_config()
    for name in ("phase1_hand_lrs", "phase2_hand_lrs", "obj_lrs", "obj_2half_lrs"):
        setattr(cfg, name, {k: v / 500.0 for k, v in getattr(cfg, name).items()})
    cfg.noise_obj_lr1, cfg.noise_obj_lr2 = cfg.noise_obj_lr1 / 500.0, cfg.noise_obj_lr2 / 500.0
    got, g, st = run(config=cfg, final_decode="hierarchical", final_extract="sparse")
    assert checked == [32] and g.count(32) == 0
    assert st["final_extract"]["vertices"] == got[0].verts_packed().shape[0] and st["inner_iterations"] > 0


@gpu
def test_call_batch_final_extract_matches_the_single_image_calls(tmp_path, monkeypatch):
    """call_batch with two images and final_extract="sparse".  Bit for bit: each image's sparse mesh equals the dense extraction of the very
    same field (checked inside the run) and the meshes of the same call_batch with the default extractor.  Against each image's
    single-image `__call__` the comparison is tests/test_pipeline.py::test_call_batch_equals_two_single_image_calls' own: equal face
    count, hand vertices within 5e-5 and object vertices within 2e-4 -- `__call__` runs the DiT, the conditioner and the VAE transformer
    on one image and call_batch runs them on two, so the FIELDS of the two routes are not the same bits (with either extractor), and the
    extractor cannot be asked for more than the fields give.  That cause is asserted: the single-image calls under the default extractor
    equal those under the sparse one bit for bit, and so do the batches.  Measured on an MI355X: equal face counts (5152, 5176), object
    vertices differing by 7.0e-6 and 8.3e-6 between `__call__` and call_batch, hand vertices by 0.  The differences are printed before
    anything is asserted."""
    pipe, img, paths, kw, _ = _pipeline_setup(tmp_path)
    hs = dict(final_extract="sparse", final_decode="hierarchical")
    singles = [pipe(image=[img], mc_algo="mc", generator=torch.Generator().manual_seed(seed), sil_renderer=None, **hs, **kw, **paths)
               for seed in (2, 3)]
    # the cause asserted: under the DEFAULT extractor and decode the single-image calls give the same bits as under the sparse one, and so
    # does the batch (below), so single vs batch is a property of the two routes' fields, the same with either extractor
    singles_default = [pipe(image=[img], mc_algo="mc", generator=torch.Generator().manual_seed(seed), sil_renderer=None, **kw, **paths)
                       for seed in (2, 3)]
    for b in range(2):
        _mesh_equal(singles_default[b], singles[b])
    grids = _GridCalls(monkeypatch)
    checked = []
    orig = ops.flexicubes_sparse

    def spy(axes, s, res, return_stats=False):
        out = orig(axes, s, res, return_stats=return_stats)
        xyz, _, _ = generate_dense_grid_points(np.full(3, -1.10), np.full(3, 1.10), octree_depth=5, octree_resolution=res, indexing="ij")
        v0, f0, l0 = ops.flexicubes(torch.as_tensor(xyz, dtype=torch.float32, device=s.device), s, res)
        checked.append(bool(v0.shape[0] > 100 and torch.equal(v0, out[0]) and torch.equal(f0, out[1]) and torch.equal(l0, out[2])))
        return out

    def batch(**extra):
        gens = [torch.Generator().manual_seed(2), torch.Generator().manual_seed(3)]
        return pipe.call_batch([img, img], [paths, paths], generators=gens, **kw, **extra)

    monkeypatch.setattr(ops, "flexicubes_sparse", spy)
    both = batch(**hs)
    monkeypatch.setattr(ops, "flexicubes_sparse", orig)
    n_grids_sparse = grids.res.count(32)
    fe = pipe.stats["final_extract"]
    grids.res.clear()
    dense = batch()
    n_grids_dense, dense_stats = grids.res.count(32), dict(pipe.stats)
    for b in range(2):
        (o1, h1), (o2, h2) = singles[b], both[b]
        same_faces = o1.faces_packed().shape == o2.faces_packed().shape
        print(f"image {b}: single vs batch faces {tuple(o1.faces_packed().shape)} {tuple(o2.faces_packed().shape)}, max |d object verts| "
              f"{float((o1.verts_packed() - o2.verts_packed()).abs().max()) if same_faces and o1.verts_packed().shape == o2.verts_packed().shape else None}, "
              f"max |d hand verts| {float((h1.verts_packed() - h2.verts_packed()).abs().max())}")
    assert n_grids_sparse == 0 and checked == [True, True]
    assert isinstance(fe, list) and len(fe) == 2
    assert n_grids_dense == 1 and "final_extract" not in dense_stats
    for b in range(2):
        _mesh_equal(dense[b], both[b])
        assert fe[b]["vertices"] == both[b][0].verts_packed().shape[0] and fe[b]["faces"] == both[b][0].faces_packed().shape[0]
    assert not torch.equal(both[0][0].verts_packed()[:50], both[1][0].verts_packed()[:50])       # two different images' meshes
    for b in range(2):
        (o1, h1), (o2, h2) = singles[b], both[b]
        assert torch.allclose(h1.verts_packed(), h2.verts_packed(), atol=5e-5)
        assert o1.faces_packed().shape == o2.faces_packed().shape and torch.allclose(o1.verts_packed(), o2.verts_packed(), atol=2e-4)
