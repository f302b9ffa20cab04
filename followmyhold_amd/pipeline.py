"""Guided flow-matching shape pipeline: the `__call__` of the reference's patched
`Hunyuan3DDiTFlowMatchingPipeline_main` (third_party_patches/hy3dgen/shapegen/pipelines.py:1041-1679; PL below) with the
optimisation-in-the-loop arithmetic on the MI355X kernels.

What stays PyTorch-ROCm ("host code stays Python"): the DiT (`model`), the ShapeVAE (`vae`: latent ->
transformer -> cross-attention geometry decoder), the image conditioner and the flow-matching scheduler.  They are
constructor arguments with the interfaces the reference uses (PL:563-742); `from_hy3dgen` adopts the components of an
installed Hunyuan3D-2 pipeline object.  What runs on hand-written HIP: FlexiCubes (`foho_flexi_fwd/_bwd`), the topology
tables of the mesh it emits (`foho_topology_tables`), and the whole guidance iteration -- transforms, three renders,
keypoints, nearest neighbours, edge loss, inside count, every loss head, their backward and the Adam/AdamW update of the
14 similarity parameters (`foho_step_run`).  Per inner iteration the only torch autograd left is
latent -> VAE -> SDF, which receives dL/dSDF from the FlexiCubes backward kernel and carries it to `noise_pred_obj`
(PL:1507-1509, PL:1600-1601).

Differences from the reference, all outside the arithmetic:
  * `renderer` / `sil_renderer` only supply the camera (fov); the fused step renders itself.
  * debug dumps (`FOHO_DEBUG_DIR`, PL:1076-1091, 1664-1675) write losses.txt / params.json and the final meshes; the
    matplotlib grids are not produced.
  * the 14 similarity parameters live in the GuidanceBatch (device memory) instead of seven leaf tensors; each phase gets
    a fresh optimiser state exactly like the reference's per-step `torch.optim.Adam/AdamW(...)` (PL:1318, 1384, 1478).
    `noise_pred_obj` keeps its own torch AdamW with the same hyper-parameters (Adam is element-wise, so splitting one
    optimiser into two changes nothing).
"""
import collections
import contextlib
import datetime
import json
import os
from typing import Optional

import numpy as np
import torch

from . import engine as E
from . import inputs, ops
from .facade import Meshes, TexturesVertex, generate_dense_grid_points, quaternion_to_matrix
from .scheduler import retrieve_timesteps


def vae_attention_backend():
    """Context for the ShapeVAE transformer's forward (and the backward recorded under it).  At the transformer's shape -- (1, 16 heads,
    3072 tokens, 64) fp16, sixteen layers, run and back-propagated in every inner iteration (PL:295, 1391-1393, 1507-1509) -- torch's
    scaled_dot_product_attention is a quarter of an iteration: forward + backward per layer on an MI355X 509-548 us with ROCm's default
    (flash, AOTriton) backend, 350 us with the memory-efficient one (139 forward, 212 backward: `vae_attention` bench record).
    This is the FALLBACK route: with `vae_transformer.install(vae)` (what `from_hy3dgen` does) the whole transformer runs on foho_vae_fwd / _bwd
    and no torch attention is called.  FOHO_VAE_SDPA selects, for a VAE that stays on its torch module:
      hip (default)  forward AND backward on this package's attention kernels (followmyhold_amd.sdpa: 71 us forward, operands read where the
                     projections left them; backward 190 us, dK / dV written directly); calls the kernels do not take (a mask, another head size)
                     and everything outside this context stay torch's, with the memory-efficient backend preferred;
      hip_torch_bwd  the HIP forward with torch's memory-efficient backward fed from it (a private torch operator: 181 us; round 5's default);
      hip_bwd        = hip (the name of round 5);
      efficient      torch's memory-efficient backend first, the others allowed behind it;
      default        torch's own choice, as the reference runs."""
    mode = os.environ.get("FOHO_VAE_SDPA", "hip")
    if mode not in ("efficient", "hip", "hip_bwd", "hip_torch_bwd") or not torch.cuda.is_available():
        return contextlib.nullcontext()
    stack = contextlib.ExitStack()
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel
        stack.enter_context(sdpa_kernel([SDPBackend.EFFICIENT_ATTENTION, SDPBackend.FLASH_ATTENTION, SDPBackend.MATH], set_priority=True))
    except (ImportError, TypeError):       # an older torch without the priority form: its own choice
        pass
    if mode != "efficient":
        from . import sdpa
        stack.enter_context(sdpa.hip_sdpa(backward="torch" if mode == "hip_torch_bwd" else "hip"))
    return stack


def vae_tokens(vae, latents):
    """`vae(latents)` of PL:295 (ShapeVAE.forward: post_kl -> transformer).  With `vae_transformer.install(vae)` the transformer -- and, under
    autograd, its backward to the latents (PL:1391-1393, 1507-1509) -- runs on this package's kernels (`foho_vae_fwd/_bwd`); inputs they do
    not take (another dtype, a token count that is not a multiple of 128) and VAEs without it go through the torch module, with the
    attention backend of `vae_attention_backend()`."""
    tr = getattr(vae, "hip_transformer", None)
    if tr is not None:
        x0 = vae.post_kl(latents)
        if tr.accepts(x0):
            return tr(x0)
    with vae_attention_backend():
        return vae(latents)


def latent2sdf(pred, xyz_samples, grid_size, vae, device, num_chunks=8000):
    """PL:292-338 (return_mesh=False): rescale the latent, run the VAE transformer, query the geometry decoder in chunks of
    8000 grid points, negate the logits so that the field is negative inside.  -> (1, G, G, G) float32."""
    pred = 1 / vae.scale_factor * pred
    pred = vae_tokens(vae, pred)
    hip = getattr(vae, "hip_geo", None)          # geo_decode.install(vae): the decoder on the matrix cores
    if hip is not None:
        # all grid points in one call, no 8000-query chunks; under autograd (PL:1391-1393, 1507-1509) the gradient reaches
        # `pred` through foho_geo_decode_bwd
        grid_logits = hip(hip.grid_queries(xyz_samples), pred)      # fp16 query points like PL:303; the query side is cached per grid
        return -grid_logits.view((1, grid_size[0], grid_size[1], grid_size[2])).float()
    logits = []
    for start in range(0, xyz_samples.shape[0], num_chunks):
        queries = xyz_samples[start:start + num_chunks].to(device).half()      # fp16 whatever the VAE's dtype (PL:303)
        logits.append(vae.geo_decoder(queries.unsqueeze(0), pred))
    grid_logits = torch.cat(logits, dim=1)
    return -grid_logits.view((1, grid_size[0], grid_size[1], grid_size[2])).float()


def _mode(value, env_name, choices, label):
    """An option switch: `value`, else $`env_name`, else "dense"; one of `choices`."""
    value = value if value is not None else (os.environ.get(env_name) or "dense")
    if value not in choices:
        raise E.L.FohoError(f"{label} {value!r}: one of {choices}")
    return value


FINAL_DECODES = ("dense", "hierarchical")


def final_decode_mode(mode=None):
    """The final decode's mode: `mode`, else $FOHO_FINAL_DECODE, else "dense" (volume.py: "hierarchical" queries the grid only near
    the surface, with a mesh identical to the dense one's for every surface the coarse level sees)."""
    return _mode(mode, "FOHO_FINAL_DECODE", FINAL_DECODES, "final_decode")


FINAL_EXTRACTS = ("dense", "sparse")


def final_extract_mode(mode=None):
    """The final step's extractor: `mode`, else $FOHO_FINAL_EXTRACT, else "dense" (ops.flexicubes on the dense point grid).  "sparse" is
    sparse_flexi.flexicubes_sparse on per-axis tables: the same mesh bit for bit, and with final_decode="hierarchical" the final
    dense point grid is never built."""
    return _mode(mode, "FOHO_FINAL_EXTRACT", FINAL_EXTRACTS, "final_extract")


GUIDANCE_EXTRACTS = ("dense", "sparse")


def guidance_extract_mode(mode=None):
    """The extractor of the guidance loop's exact-size path: `mode`, else $FOHO_GUIDANCE_EXTRACT, else "dense" (ops.flexicubes on the
    dense point grid).  "sparse" is sparse_flexi.flexicubes_sparse_grad on per-axis tables: the same mesh bit for bit, work and memory
    proportional to the surface cubes, and a dL/dSDF that is bitwise repeatable.  Capacity mode (engine.SdfObjective) is untouched."""
    return _mode(mode, "FOHO_GUIDANCE_EXTRACT", GUIDANCE_EXTRACTS, "guidance_extract")


GUIDANCE_DECODES = ("dense", "hierarchical")


def guidance_decode_mode(mode=None):
    """How the guidance grid is decoded -- the in-loop decodes of phases B / C and the per-step decodes before the last step: `mode`,
    else $FOHO_GUIDANCE_DECODE, else "dense".  "hierarchical" is the band decode of latent2sdf_band."""
    return _mode(mode, "FOHO_GUIDANCE_DECODE", GUIDANCE_DECODES, "guidance_decode")


def _require_decoder(vae, which):
    """vae.hip_geo for the hierarchical decode of the `which` ("final" | "guidance") grid; the guidance grid's band decode runs under
    autograd and so also needs a backward that does not keep every forward row."""
    hip = getattr(vae, "hip_geo", None)
    if hip is None:
        raise E.L.FohoError(f"hierarchical {which} decode: needs vae.hip_geo, the HIP geometry decoder (geo_decode.install(vae)); the torch "
                            "module's outputs depend on the batch shape, so decoded subsets would not equal the dense decode")
    if which == "guidance" and hip.backward_mode == "keep":
        raise E.L.FohoError("hierarchical guidance decode: vae.hip_geo.backward_mode 'keep' keeps the activations of every forward row and "
                            "cannot serve a band decode: use 'rows' (the default) or 'recompute'")
    return hip


def sdf_hierarchical_from_tokens(tokens, bmin, bmax, res, hip, min_res=None, band=1):
    """The hierarchical decode of one image's VAE tokens (1, L, width) -> ((1, G, G, G) float32 negated logits, stats).  Every query
    goes through `hip(queries, tokens)` exactly as latent2sdf's dense call does: K / V prepared once for the tokens, the logits in
    the tokens' dtype -- so the decoded values equal the dense decode's bit for bit."""
    from . import volume
    res = int(res)
    G = res + 1
    with torch.no_grad():
        logits, stats = volume.hierarchical_grid_logits(lambda q: hip(q.reshape(1, -1, 3), tokens).reshape(-1).float(), bmin, bmax, res,
                                                        min_res=min_res, band=band, device=hip.device)
    return -logits.view(1, G, G, G), stats


def latent2sdf_hierarchical(pred, bmin, bmax, res, vae, device, min_res=None, band=1):
    """latent2sdf with the hierarchical decode (volume.hierarchical_grid_logits) on the (res+1)^3 grid over [bmin, bmax]: the tokens
    once, as latent2sdf computes them, then the HIP geometry decoder on the gathered query points of each level.
    -> ((1, G, G, G) float32, negative inside, stats).  Requires `vae.hip_geo`."""
    from . import volume
    volume.check_levels(res, min_res)
    hip = _require_decoder(vae, "final")
    pred = vae_tokens(vae, 1 / vae.scale_factor * pred)
    return sdf_hierarchical_from_tokens(pred, bmin, bmax, res, hip, min_res=min_res, band=band)


def guidance_levels(res, min_res=None):
    """(res, min_res) of the guidance grid's band decode after volume.check_levels.  min_res defaults to res / 2 (33^3 at level 0 of
    the 65^3 grid), not the final decode's res / 4: a surface component inside one-sign coarse cells is missed, and in the loop that
    changes the losses -- a 17^3 level 0 has 0.1375-unit cells, wide enough to hide a mug handle."""
    from . import volume
    res = int(res)
    return volume.check_levels(res, res // 2 if min_res is None else min_res)


def sdf_band_from_tokens(tokens, xyz_samples, res, hip, bmin, bmax, min_res=None, band=1):
    """The band decode of B images' VAE tokens (a list of (1, L, width) tensors) on the grid `xyz_samples` of resolution `res` over
    [bmin, bmax] -> ((B, (res+1)^3) float32 negated logits, list of B stats, host reads).  The images step through the levels in
    lockstep with one host read per level and per closure round (volume.hierarchical_grid_logits_batch).

    Under autograd (a token tensor that requires grad) the decode is geo_decode._GeoBandFn on each image's `hip.kv_of(tokens)`: the
    logits' gradient reaches the tokens through the dense route's backward on the full grid, bitwise the dense route's for the same
    incoming gradient.  Without it every query goes through `hip(queries, tokens)` as latent2sdf's no-gradient call does.  Either way
    a decoded value equals the dense route's bit for bit, and the field is the dense one's everywhere FlexiCubes reads a value."""
    from . import geo_decode, volume
    res, min_res = guidance_levels(res, min_res)
    n = (res + 1) ** 3
    if xyz_samples.shape[0] != n:
        raise E.L.FohoError(f"band decode: {xyz_samples.shape[0]} grid points, a grid of resolution {res} has {n}")
    if not tokens:
        return torch.empty(0, n, device=hip.device), [], 0
    dtype = tokens[0].dtype
    box = {}

    def run(decodes):
        fields, box["stats"], box["reads"] = volume.hierarchical_grid_logits_batch(decodes, bmin, bmax, res, min_res=min_res, band=band,
                                                                                   device=hip.device)
        return fields

    queries = hip.grid_queries(xyz_samples)          # the dense route's query tensor: what the backward runs on
    if torch.is_grad_enabled() and any(t.requires_grad for t in tokens):      # _GeoBandFn refuses backward_mode "keep"
        logits = geo_decode._GeoBandFn.apply(queries, hip, run, dtype, *[hip.kv_of(t) for t in tokens])
    else:
        with torch.no_grad():
            logits = torch.stack(run([lambda p, t=t: hip(p.reshape(1, -1, 3), t).reshape(-1).float() for t in tokens]))
    return (-logits.to(dtype)).float(), box["stats"], box["reads"]


def latent2sdf_band(pred, xyz_samples, grid_size, vae, device, bmin, bmax, min_res=None, band=1):
    """latent2sdf with the band decode (volume.hierarchical_grid_logits), with or without gradient: the tokens once, as latent2sdf
    computes them, then the HIP geometry decoder on each level's gathered points of the grid `xyz_samples` over [bmin, bmax].
    -> ((1, G, G, G) float32, negative inside, stats).  Requires `vae.hip_geo` in backward_mode "rows" or "recompute".

    The one behavioural difference from latent2sdf: a NaN that the decoder would produce only at points the band fills is not seen."""
    G = int(grid_size[0])
    guidance_levels(G - 1, min_res)
    hip = _require_decoder(vae, "guidance")
    pred = vae_tokens(vae, 1 / vae.scale_factor * pred)
    sdf, stats, _ = sdf_band_from_tokens([pred], xyz_samples, G - 1, hip, bmin, bmax, min_res=min_res, band=band)
    return sdf.view(1, G, G, G), stats[0]


def _tally(entry, st):
    """Add one band decode's stats to stats["guidance_decode"] (one image's entry)."""
    n = entry.get("decodes", 0)
    entry.update(decodes=n + 1, levels=st["levels"],
                 mean_decoded_fraction=(entry.get("mean_decoded_fraction", 0.0) * n + st["decoded_fraction"]) / (n + 1),
                 max_decoded_fraction=max(entry.get("max_decoded_fraction", 0.0), st["decoded_fraction"]),
                 max_closure_rounds=max(entry.get("max_closure_rounds", 0), st["closure_rounds"]),
                 fallbacks=entry.get("fallbacks", 0) + int(st["fallback"]))


def _bound_active_rows(vae, n_rows):
    """The decoder's active-row backward (foho_geo_decode_bwd_rows) launches row blocks up to an upper bound of the rows that carry a
    gradient; every block beyond the actual count is fourteen empty launches (4.5 us each).  In the guidance loop the gradient comes
    out of the FlexiCubes backward, which has run by the time the iteration's flags are read back: `n_rows` = the exact count
    (SdfObjective.active_rows(), or a surface's face count on the exact-size path: one quad per crossed edge).  Returns the decoder
    (or None) so that the caller can check `rows_dropped` when the phase is over -- a safety net that never fires with an exact count."""
    hip = getattr(vae, "hip_geo", None)
    if hip is not None:
        hip.row_cap = max(int(n_rows), 1)
    return hip


def _check_rows_dropped(hip):
    """End of a phase: did ANY backward of it (every iteration, every image of a batch) drop rows?  Also lifts the bound again -- `row_cap`
    is state on the shared decoder, and a backward outside the loop (a dense gradient from user code) must not inherit the last
    iteration's count."""
    if hip is not None:
        cap, hip.row_cap = hip.row_cap, None
        dropped = hip.take_rows_dropped()
        if dropped:
            raise E.L.FohoError(f"geometry decoder backward: {dropped} active rows exceeded row_cap (last: {cap}) during this phase: its gradient "
                                "is incomplete (raise obj_capacity or leave vae.hip_geo.row_cap = None)")


@contextlib.contextmanager
def _latent_phase_scope(hip):
    """One latent phase (B / C) of either driver on the shared decoder `hip` (vae.hip_geo, or None).  However the phase ends -- a NaN
    return, an exception --, neither the active-row bound nor a dropped-row count outlives it: the count of a phase that never reached
    its own _check_rows_dropped must not fail the next phase's."""
    try:
        yield
    finally:
        if hip is not None:
            hip.row_cap = None
            hip.take_rows_dropped()


def similarity_about_center(verts, scale, quat, trans):
    """transform_mesh_around_center_w_scale (PL:108-118): scale and rotate about the bounding-box centre, then shift."""
    center = (verts.min(dim=0)[0] + verts.max(dim=0)[0]) / 2.0
    R = quaternion_to_matrix(quat).float().reshape(3, 3)
    return (scale * (verts - center)) @ R.T + center + trans


def _cat_recursive(*parts, dtype):
    if isinstance(parts[0], torch.Tensor):
        return torch.cat(parts, dim=0).to(dtype)
    return {k: _cat_recursive(*[p[k] for p in parts], dtype=dtype) for k in parts[0].keys()}


class BatchLeftFastPath(RuntimeError):
    """An image of a `call_batch` batch needs the per-image handling of `__call__` (a non-manifold or over-capacity iso-surface, a
    NaN loss).  `call_batch` does not raise it: the image's entry of the result list IS an instance (with `.phase`, `.step`,
    `.iteration`, `.flags`), the other images of the batch carry on, and the caller re-runs that image through `__call__`."""

    def __init__(self, msg, phase=None, step=None, iteration=None, flags=0):
        super().__init__(msg)
        self.phase, self.step, self.iteration, self.flags = phase, step, iteration, flags


# ---------------------------------------------------------------------- what `__call__` and `call_batch` share
_Options = collections.namedtuple("_Options", "final_mode final_min_res final_sparse guid_band guid_min_res")
_OPTION_KWARGS = ("final_decode", "final_decode_min_res", "final_extract", "guidance_decode", "guidance_decode_min_res")
_Schedule = collections.namedtuple("_Schedule", "do_cfg cond bmin bmax xyz timesteps n_steps_obj guidance")


def _schedule_options(vae, guid_res, final_res, final_decode, final_decode_min_res, final_extract, guidance_decode, guidance_decode_min_res):
    """The drivers' option switches (arguments in the order of _OPTION_KWARGS), parsed and then validated against the grids and the VAE:
    a bad one is refused before any work, not after the whole schedule."""
    final_mode = final_decode_mode(final_decode)
    final_sparse = final_extract_mode(final_extract) == "sparse"
    guid_band = guidance_decode_mode(guidance_decode) == "hierarchical"
    if final_mode == "hierarchical":
        from . import volume
        volume.check_levels(final_res, final_decode_min_res)
        _require_decoder(vae, "final")
    if guid_band:
        guidance_levels(guid_res, guidance_decode_min_res)
        _require_decoder(vae, "guidance")
    return _Options(final_mode, final_decode_min_res, final_sparse, guid_band, guidance_decode_min_res)


def _grid_points(bmin, bmax, res, device):
    """The dense point grid the latent is decoded on (PL:1126-1143); FlexiCubes needs no cube index table here."""
    xyz_np, _, _ = generate_dense_grid_points(bmin, bmax, octree_depth=5, octree_resolution=res, indexing="ij")
    return torch.as_tensor(xyz_np, dtype=torch.float32, device=device)


def _load_scenes(paths, fovs, J_regressor, device):
    """Per-image inputs (PL:1217-1256): masks, keypoints, aligned MANO mesh, Hunyuan -> MoGe transform, MoGe target maps.  paths: per image
    a dict with the reference's eight path names (fov.json lies next to the MoGe mesh); fovs: per image degrees, or None for its fov.json;
    J_regressor: None for the file of PL:1218.  -> (scenes, T_h2m, hand_verts, hand_faces), the last three per image on the device."""
    jr = inputs.load_j_regressor() if J_regressor is None else np.asarray(J_regressor, np.float32)
    scenes = []
    for p, fov in zip(paths, fovs):
        q = dict(cropped_hand_mask_path=p["hand_mask_path"], cropped_obj_mask_path=p["obj_mask_path"], moge_mesh_path=p["moge_mesh_path"],
                 moge_fov_path=os.path.join(os.path.dirname(p["moge_mesh_path"]), "fov.json"), T_h2m_path=p["h2m_rt_path"],
                 aligned_mano_mesh_path=p["aligned_mano_mesh_path"], hamer_for_guid_path=p["hamer_for_guid_path"])
        scenes.append(inputs.load_scene_from_files(q, jr, E.hip_render_fn(device), fov=fov, with_object=False))
    on_device = lambda key, dtype: [torch.as_tensor(sc[key], dtype=dtype, device=device) for sc in scenes]
    return scenes, on_device("T_h2m", torch.float32), on_device("hand_verts", torch.float32), on_device("hand_faces", torch.int64)


def _hand_phase(gb, cfg0, i, stats, device, spg=None, after_capture=None, before_replay=None):
    """Phase A: hands only, no latent involved (PL:1296-1358): optimization_steps_hand fused steps as replays of one captured graph of
    `spg` steps (default: the largest divisor of the count up to 50).  after_capture() runs between the capture and the first replay,
    before_replay(rep) in front of each replay.  -> the flags raise_on_flags returns."""
    cfg, n_renders = E.phase_cfg("A", cfg0, denoise_i=i, do_update=True)
    gb.set_n_renders(n_renders)
    gb.reset_optimizer()
    n = int(cfg0.optimization_steps_hand)
    if spg is None:
        spg = max([d for d in range(1, 51) if n % d == 0]) if n > 0 else 1
    graph = gb.capture(cfg, steps_per_graph=spg)
    if after_capture is not None:
        after_capture()
    gb.reset_optimizer()
    for rep in range(n // spg):
        if before_replay is not None:
            before_replay(rep)
        graph.replay()
    stats["inner_iterations"] += n
    torch.cuda.synchronize(device)
    return gb.raise_on_flags(strict_k=False)


class _StepDecoder:
    """Every decode of one driver call, at the level of VAE tokens: `vae_tokens` runs once for all images of the call, then each live image
    goes through the HIP decoder (gradients through foho_geo_decode_bwd) or through the torch module in chunks of `num_chunks` queries; a
    frozen slot (`frozen`: call_batch's images that left the batch) is not decoded any more and gets the all-ones field: no surface.  An
    image's values are those latent2sdf, latent2sdf_band and latent2sdf_hierarchical compute for it.  Fills stats["guidance_decode"],
    stats["final_decode"] and stats["final_extract"]: one entry for `__call__`, a list per image for call_batch (`per_image`)."""

    def __init__(self, vae, sch, opts, guid_res, final_res, stats, num_chunks, n_images=1, frozen=(), per_image=False):
        self.vae, self.sch, self.opts, self.guid_res, self.final_res, self.stats = vae, sch, opts, guid_res, final_res, stats
        self.num_chunks, self.n_images, self.frozen, self.per_image = num_chunks, n_images, frozen, per_image

    def _open(self, key):
        if self.per_image:
            self.stats[key] = [None] * self.n_images

    def _record(self, key, b, value):
        if self.per_image:
            self.stats[key][b] = value
        else:
            self.stats[key] = value

    def guidance(self, x1):
        """The fields of latents x1 (B, ...) on the guidance grid, a list of B ((guid_res+1)^3,) tensors: dense, or the band decode with
        the live images in lockstep (sdf_band_from_tokens), either with or without gradient."""
        return self._fields(x1, self.guid_res, self.sch.xyz, "band" if self.opts.guid_band else "dense")

    def step_grid(self, last):
        """The grid a step's clean-sample estimate is decoded on and its extractor -> (res, points or None, extract(field, b) -> (verts,
        faces)): the guidance grid before the last step (those meshes only matter as the fall-back of a later empty decode), the final
        grid at the last one (PL:1626-1642) -- whose points neither a hierarchical decode nor the sparse extractor reads."""
        sch, opts = self.sch, self.opts
        res = self.final_res if last else self.guid_res
        sparse = last and opts.final_sparse
        if res == self.guid_res:
            xyz = sch.xyz
        else:
            xyz = None if sparse and opts.final_mode == "hierarchical" else _grid_points(sch.bmin, sch.bmax, res, sch.xyz.device)
        if not sparse:
            return res, xyz, lambda s, b: ops.flexicubes(xyz, s, res)[:2]
        axes = ops.grid_axes(sch.bmin, sch.bmax, res).to(sch.xyz.device)      # the final step's mesh from axis tables
        self._open("final_extract")

        def extract(s, b):
            v, f, _, st = ops.flexicubes_sparse(axes, s, res, return_stats=True)
            self._record("final_extract", b, st)
            return v, f

        return res, xyz, extract

    def step(self, x1, last, res, xyz):
        """The fields of a step's clean-sample estimates x1 on step_grid(last)'s grid, a list of B ((res+1)^3,) tensors without gradient:
        the last step's dense or near the surface only (volume.py), an earlier step's as guidance() decodes."""
        if last:
            return self._fields(x1, res, xyz, "hierarchical" if self.opts.final_mode == "hierarchical" else "dense")
        return self.guidance(x1)

    def _fields(self, x1, res, xyz, mode):
        vae, sch, hip = self.vae, self.sch, getattr(self.vae, "hip_geo", None)
        tokens = vae_tokens(vae, 1 / vae.scale_factor * x1)          # all images through ONE foho_vae_fwd (rows = images x tokens)
        n = (res + 1) ** 3
        live = [b for b in range(x1.shape[0]) if b not in self.frozen]
        out = [torch.ones(n, device=x1.device) if b in self.frozen else None for b in range(x1.shape[0])]
        if mode == "band":
            sdf, sts, _ = sdf_band_from_tokens([tokens[b:b + 1] for b in live], xyz, res, hip, sch.bmin, sch.bmax, min_res=self.opts.guid_min_res)
            for j, b in enumerate(live):
                out[b] = sdf[j]
                _tally(self.stats["guidance_decode"][b] if self.per_image else self.stats["guidance_decode"], sts[j])
        elif mode == "hierarchical":
            self._open("final_decode")
            for b in live:
                sdf_b, st = sdf_hierarchical_from_tokens(tokens[b:b + 1], sch.bmin, sch.bmax, res, hip, min_res=self.opts.final_min_res)
                out[b] = sdf_b.view(-1)
                self._record("final_decode", b, st)
        else:
            for b in live:
                if hip is not None:          # geo_decode.install(vae): all grid points in one call, fp16 query points like PL:303
                    out[b] = -hip(hip.grid_queries(xyz), tokens[b:b + 1]).view(-1).float()
                    continue
                logits = [vae.geo_decoder(xyz[s0:s0 + self.num_chunks].half().unsqueeze(0), tokens[b:b + 1]) for s0 in range(0, n, self.num_chunks)]
                out[b] = -torch.cat(logits, dim=1).view(-1).float()
        return out


def _single_colour(verts, faces, channel):
    tex = torch.zeros_like(verts)
    tex[:, channel] = 1.0
    return Meshes(verts=[verts], faces=[faces], textures=TexturesVertex(verts_features=[tex]))


def _meshes_in_moge_world(verts, faces, T_h2m, p, hand_verts, hand_faces, with_hand):
    """A step's clean-sample estimate in the MoGe world (PL:1612-1661) from the extracted mesh, the Hunyuan -> MoGe transform, the 16
    similarity parameters `p` and the MoGe-space MANO mesh -> (blue object Meshes, or None for an empty mesh; green hand Meshes, or None
    without `with_hand`).  The hand is THIS step's whatever the decode gives: PL:1615-1619 come before the empty-mesh test of PL:1644-1646."""
    obj = hand = None
    if with_hand:
        hand = _single_colour(similarity_about_center(hand_verts, p[0], p[4:8], p[1:4]), hand_faces, 1)
    if verts.shape[0] == 0:
        print("Invalid mesh detected, aborting step!")
    else:
        obj = _single_colour(similarity_about_center(verts @ T_h2m[:3, :3].T + T_h2m[:3, 3], p[8], p[12:16], p[9:12]), faces, 2)
    return obj, hand


class GuidedShapePipeline:
    """Drop-in for `Hunyuan3DDiTFlowMatchingPipeline_main`: same constructor (PL:563-585), same `__call__` signature and
    return value (PL:1044-1072, 1679)."""

    def __init__(self, vae, model, scheduler, conditioner, image_processor, device="cuda", dtype=torch.float16, **kwargs):
        self.vae, self.model, self.scheduler = vae, model, scheduler
        self.conditioner, self.image_processor = conditioner, image_processor
        # The guidance optimises the noise prediction and fourteen pose parameters (PL:1318, 1384, 1478), never a network weight: with
        # the weights' requires_grad left at torch's default the backward of every inner iteration would also form d loss / d W of
        # the whole ShapeVAE transformer -- as much matrix work again as the gradient that is wanted -- into .grad buffers nobody reads.
        for net in (vae, model, conditioner):
            if isinstance(net, torch.nn.Module):
                net.requires_grad_(False)
        self.to(device, dtype)

    @classmethod
    def from_hy3dgen(cls, pipe, hip_geo_decoder=True, hip_vae_transformer=True):
        """Adopt the networks of an (unpatched) hy3dgen `Hunyuan3DDiTFlowMatchingPipeline` object.  The ShapeVAE's geometry
        decoder -- the 65^3-point decode and its backward inside every inner iteration, PL:292-313, 1391-1393, 1507-1509 -- is
        taken over by the matrix-core kernels (`geo_decode.install`), and so is the transformer in front of it (`vae(pred)`, PL:295:
        `vae_transformer.install`); a module outside the shapes / layouts they take raises `FohoError` here,
        `hip_geo_decoder=False` / `hip_vae_transformer=False` keep the torch modules."""
        from .scheduler import FlowMatchEulerDiscreteScheduler
        sch = FlowMatchEulerDiscreteScheduler(num_train_timesteps=pipe.scheduler.config.num_train_timesteps,
                                              shift=getattr(pipe.scheduler.config, "shift", 1.0))
        self = cls(pipe.vae, pipe.model, sch, pipe.conditioner, pipe.image_processor, device=pipe.device, dtype=pipe.dtype)
        if hip_geo_decoder:
            from . import geo_decode
            geo_decode.install(self.vae, device=self.device)
        if hip_vae_transformer:
            from . import vae_transformer
            vae_transformer.install(self.vae, device=self.device)
        return self

    def to(self, device=None, dtype=None):
        if device is not None:
            self.device = torch.device(device)
            for m in (self.vae, self.model, self.conditioner):
                m.to(device)
        if dtype is not None:
            self.dtype = dtype
            for m in (self.vae, self.model, self.conditioner):
                m.to(dtype=dtype)

    # ------------------------------------------------------------------ PL:599-742
    def encode_cond(self, image, mask, do_classifier_free_guidance, dual_guidance, to_cpu=False):
        bsz = image.shape[0]
        cond = self.conditioner(image=image, mask=mask)
        if do_classifier_free_guidance:
            un_cond = self.conditioner.unconditional_embedding(bsz)
            if dual_guidance:
                drop_main = dict(un_cond)
                drop_main["additional"] = cond["additional"]
                cond = _cat_recursive(cond, drop_main, un_cond, dtype=self.dtype)
            else:
                cond = _cat_recursive(cond, un_cond, dtype=self.dtype)
        if to_cpu:
            self.conditioner.to("cpu")
        return cond

    def prepare_latents(self, batch_size, dtype, device, generator, latents=None):
        shape = (batch_size, *self.vae.latent_shape)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective "
                             f"batch size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            gdev = generator.device if isinstance(generator, torch.Generator) else device
            latents = torch.randn(shape, generator=generator if isinstance(generator, torch.Generator) else None,
                                  device=gdev, dtype=dtype).to(device)
        else:
            latents = latents.to(device)
        return latents * getattr(self.scheduler, "init_noise_sigma", 1.0)

    def prepare_image(self, image, hand_mask=None):
        if isinstance(image, str) and not os.path.exists(image):
            raise FileNotFoundError(f"Couldn't find image at path {image}")
        images, masks = [], []
        for img in image if isinstance(image, list) else [image]:
            out = self.image_processor(img, return_mask=True)
            im, mk = (out.get("image"), out.get("mask")) if isinstance(out, dict) else out
            images.append(im)
            masks.append(mk)
        images = torch.cat(images, dim=0).to(self.device, dtype=self.dtype)
        masks = torch.cat(masks, dim=0).to(self.device, dtype=self.dtype) if masks[0] is not None else None
        return images, masks

    # ------------------------------------------------------------------ the schedule both drivers run
    def _schedule_setup(self, images, guidance_scale, n_images, n_steps, guid_res, sigmas=None):
        """What the denoising loop needs besides latents and scenes (PL:1100-1215): the conditioning, the guidance grid over the Hunyuan
        box, the timesteps (sigmas start from 0, PL:1186-1193) and the guidance tensor; the networks in eval mode."""
        do_cfg = guidance_scale >= 0 and not (getattr(self.model, "guidance_embed", False) is True)
        img, msk = self.prepare_image(images)
        cond = self.encode_cond(image=img, mask=msk, do_classifier_free_guidance=do_cfg, dual_guidance=False)
        bmin, bmax = np.full(3, -1.10), np.full(3, 1.10)
        xyz = _grid_points(bmin, bmax, guid_res, self.device)
        sigmas = np.linspace(0, 1, n_steps) if sigmas is None else sigmas
        timesteps, n_steps_obj = retrieve_timesteps(self.scheduler, n_steps, self.device, sigmas=sigmas)
        guidance = None
        if getattr(self.model, "guidance_embed", False) is True:
            guidance = torch.tensor([guidance_scale] * n_images, device=self.device, dtype=self.dtype)
        self.model.eval()
        self.vae.eval()
        return _Schedule(do_cfg, cond, bmin, bmax, xyz, timesteps, n_steps_obj, guidance)

    def _noise_prediction(self, sch, latents, i, t, cfg0):
        """The DiT's noise prediction at step i, with the classifier-free mix: trust the learned prior early, the guidance later
        (PL:1284-1293)."""
        latent_in = torch.cat([latents] * 2) if sch.do_cfg else latents
        timestep = t.expand(latent_in.shape[0]).to(latents.dtype) / self.scheduler.config.num_train_timesteps
        noise_pred = self.model(latent_in, timestep, sch.cond, guidance=sch.guidance)
        if sch.do_cfg:
            scale_i = cfg0.obj_guidance_scale * (1 - i / sch.n_steps_obj) if i >= cfg0.guidance_start_step + 1 else cfg0.obj_guidance_scale
            c, u = noise_pred.chunk(2)
            noise_pred = u + scale_i * (c - u)
        return noise_pred

    # ------------------------------------------------------------------ B images through one pass of the schedule
    @torch.no_grad()
    def call_batch(self, images, paths, generators=None, guidance_scale=7.5, num_chunks=8000, config=None, renderer=None,
                   J_regressor=None, guidance_octree_resolution=64, final_octree_resolution=384, obj_capacity=None, fovs=None,
                   final_decode=None, final_decode_min_res=None, guidance_decode=None, guidance_decode_min_res=None, final_extract=None):
        """`__call__` for B images at once ("within a GPU, batch the rank's images through each kernel
        launch").  The reference runs its images one after the other (RUN:208-259, batch_size = 1, guid_config.py:9); here
        one pass of the 20-step schedule serves all of them: the DiT and the ShapeVAE transformer run on B latents, the
        optimisation-in-the-loop iterations run as ONE capacity-mode GuidanceBatch of B slots -- per iteration one hipGraph
        replay of iso-surfacing, object installation, fused step and iso-surface backward for all B (engine.SdfObjective) --
        and one AdamW over the (B, L, D) noise prediction (element-wise: B independent optimisers).

        images: list of B images (as `__call__` takes one); paths: list of B dicts with `__call__`'s eight path arguments;
        generators: list of B torch.Generators (default: every image seeded with 2, RUN:120, 144); fovs: list of B fields of
        view in degrees (default: the renderer's camera for all, else each image's fov.json -- what RUN:228-230 hands to its
        camera).  All images must share H x W.  -> list of B (object Meshes, hand Meshes) in the MoGe world.

        Events the reference handles per image are handled per image here, too, with ONE read-back of the B flag words per
        iteration (the reference's NaN test is one as well): an EMPTY iso-surface skips that image's iteration -- no optimiser
        step for its noise prediction, none for its pose (PL:1394-1397, 1511-1513; `stats["skipped_empty"]`); an image whose
        surface is not a closed manifold or exceeds the capacity, or whose loss is NaN (PL:1442-1444, 1590-1592), LEAVES the batch:
        its slot is frozen, the other images carry on, and its entry of the result list is a `BatchLeftFastPath` instance -- the
        caller re-runs that image through `__call__`, which handles all of these the reference's way.

        final_decode: "dense" or "hierarchical" (None: $FOHO_FINAL_DECODE, else "dense"), with final_decode_min_res, as in `__call__`: the
        last step's grid of each image decoded densely or near the surface only (volume.py); per-image stats in stats["final_decode"].
        guidance_decode: "dense" or "hierarchical" (None: $FOHO_GUIDANCE_DECODE, else "dense"), with guidance_decode_min_res, as in
        `__call__`: every decode on the guidance grid by the band decode, all images in lockstep (sdf_band_from_tokens); per-image stats
        in stats["guidance_decode"].
        final_extract: "dense" or "sparse" (None: $FOHO_FINAL_EXTRACT, else "dense"), as in `__call__`: the last step's mesh of each image
        by ops.flexicubes on the dense point grid or by flexicubes_sparse on axis tables (the same mesh; with a hierarchical final
        decode the final point grid is not built); per-image stats in stats["final_extract"]."""
        B = len(images)
        guid_res, final_res = int(guidance_octree_resolution), int(final_octree_resolution)
        opts = _schedule_options(self.vae, guid_res, final_res, final_decode, final_decode_min_res, final_extract, guidance_decode,
                                 guidance_decode_min_res)
        device, dtype = self.device, self.dtype
        cfg0 = config() if config is not None else E.OptimizationConfig()
        self.stats = stats = {"inner_iterations": 0, "images": B, "skipped_empty": 0}
        if opts.guid_band:
            stats["guidance_decode"] = [{} for _ in range(B)]
        left = {}                 # image -> BatchLeftFastPath: frozen slots
        n_steps, hand_start = cfg0.num_inference_steps, cfg0.handopt_start_step
        sch = self._schedule_setup(list(images), guidance_scale, B, n_steps, guid_res)
        if generators is None:
            generators = [torch.Generator().manual_seed(2) for _ in range(B)]
        latents = torch.cat([self.prepare_latents(1, dtype, device, g) for g in generators], 0).clone()

        if fovs is None:
            fovs = [float(renderer.rasterizer.cameras.fov) if renderer is not None else None] * B
        scenes, T_h2m, hand_moge, hand_faces = _load_scenes(paths, fovs, J_regressor, device)
        cap = tuple(obj_capacity) if obj_capacity else (8 * guid_res * guid_res, 16 * guid_res * guid_res)
        gb = E.GuidanceBatch(scenes, device=device, grid_res=guid_res, n_renders=2, obj_capacity=cap)
        fobj = E.SdfObjective(gb, sch.xyz, guid_res)
        hip_dec = getattr(self.vae, "hip_geo", None)
        decoder = _StepDecoder(self.vae, sch, opts, guid_res, final_res, stats, num_chunks, n_images=B, frozen=left, per_image=True)

        LEAVE, EMPTY = 1 | 16 | 32, 64      # flag bits: NaN loss, capacity overflow, not a closed manifold | empty iso-surface

        def latent_phase(phase, iters, i, t, noise_pred, lr):
            cfg, n_renders = E.phase_cfg(phase, cfg0, denoise_i=i, do_update=True)
            gb.set_n_renders(n_renders)
            gb.reset_optimizer()
            for b in left:                # reset_optimizer cleared the sticky bits: a slot that left stays frozen
                gb.flags[b] |= 16
            # one leaf and one parameter group per image: torch.optim.AdamW then keeps a step count per image and skips an image
            # whose gradient is None -- the reference's `continue` in front of its optimiser step, image by image
            noise = [noise_pred[b:b + 1].clone().detach().requires_grad_(True) for b in range(B)]
            opt = torch.optim.AdamW([{"params": [n], "lr": lr} for n in noise], eps=1e-4)
            for k in range(int(iters)):
                opt.zero_grad(set_to_none=True)
                sdf = torch.stack(decoder.guidance(self.scheduler.step_final(torch.cat(noise, 0), t, latents)), 0)
                loss = fobj(sdf, cfg)                                   # (B,): one replay for all images
                fl = gb.flags.cpu().tolist()                            # the iteration's read-back (NaN is bit 0 of the flags) ...
                if hip_dec is not None:                                 # ... with the rows the decoder's backward will find a gradient on
                    _bound_active_rows(self.vae, max(fobj.active_rows()))
                go_host = [0.0] * B                                     # (host list, uploaded once: no per-image device synchronisation)
                for b in range(B):
                    if b in left:
                        continue
                    if fl[b] & LEAVE:
                        what = "a NaN loss" if fl[b] & 1 else ("an iso-surface beyond the capacity" if fl[b] & 16 else "an iso-surface that is not a closed manifold")
                        left[b] = BatchLeftFastPath(f"phase {phase}, denoising step {i}, iteration {k}: {what}", phase, i, k, fl[b])
                        gb.flags[b] |= 16                               # frozen from here on (the step leaves flagged slots alone)
                    elif fl[b] & EMPTY:
                        print("Invalid mesh detected, aborting step!")  # PL:1396, 1512
                        stats["skipped_empty"] += 1
                        gb.flags[b] &= ~EMPTY
                    else:
                        go_host[b] = 1.0
                if len(left) == B:
                    break
                go = torch.tensor(go_host, device=device)
                (loss * go).sum().backward()         # _SdfObjectiveFn.backward returns exact zeros for go = 0 (also past a NaN)
                for b in range(B):
                    if go_host[b] == 0:
                        noise[b].grad = None
                opt.step()
                stats["inner_iterations"] += 1
            gb.raise_on_flags(strict_k=False, ignore_images=list(left))
            _check_rows_dropped(hip_dec)
            return torch.cat([n.detach() for n in noise], 0).clone()

        results = [(None, None)] * B
        for i, t in enumerate(sch.timesteps):
            noise_pred = self._noise_prediction(sch, latents, i, t, cfg0)
            if i >= hand_start:
                with torch.enable_grad():
                    if i == hand_start:
                        _hand_phase(gb, cfg0, i, stats, device)
                    elif len(left) < B:                                  # (else nobody is left to optimise: the caller re-runs them all)
                        with _latent_phase_scope(hip_dec):
                            if i == hand_start + 1:                      # phase B (PL:1361-1453)
                                noise_pred = latent_phase("B", cfg0.optimization_steps_scale, i, t, noise_pred, cfg0.noise_obj_lr1)
                            else:                                        # phase C (PL:1455-1601)
                                noise_pred = latent_phase("C", cfg0.optimization_steps_joint, i, t, noise_pred, cfg0.noise_obj_lr2)
                noise_pred = noise_pred.detach().clone()
            latents = self.scheduler.step(noise_pred, t, latents).prev_sample
            # the clean-sample estimate as a mesh in the MoGe world (PL:1612-1661): the last one is the result
            last = i == n_steps - 1
            res, xyz, extract = decoder.step_grid(last)
            sdf = decoder.step(self.scheduler.step_final(noise_pred, t, latents), last, res, xyz)
            for b in range(B):
                if b not in left:
                    obj, hand = _meshes_in_moge_world(*extract(sdf[b], b), T_h2m[b], gb.params[b], hand_moge[b], hand_faces[b], i >= hand_start)
                    results[b] = (results[b][0] if obj is None else obj, results[b][1] if hand is None else hand)
        for b, why in left.items():
            results[b] = why
        self.guidance_batch = gb
        stats["left_batch"] = sorted(left)
        return results

    # ------------------------------------------------------------------ PL:1044-1679
    @torch.no_grad()
    def __call__(self, image=None, num_inference_steps: int = 30, timesteps=None, sigmas=None, eta: float = 0.0,
                 guidance_scale: float = 7.5, generator=None, box_v=1.10, octree_resolution=64, mc_level=0.0, mc_algo="mc",
                 num_chunks=8000, output_type: Optional[str] = "trimesh", enable_pbar=True, config=None, renderer=None,
                 sil_renderer=None, cropped_obj_img_path=None, hamer_for_guid_path=None, aligned_mano_mesh_path=None,
                 obj_mask_path=None, hand_mask_path=None, moge_mesh_path=None, h2m_rt_path=None, hunyuan_hoi_mesh_path=None,
                 **kwargs):
        kwargs.pop("callback", None)            # popped and ignored, as in PL:1073-1074
        kwargs.pop("callback_steps", None)
        final_res = int(kwargs.pop("final_octree_resolution", 384))          # PL:1627 (tests use a smaller grid)
        guid_res = int(kwargs.pop("guidance_octree_resolution", 64))
        # not in the signature, which is the reference's: call_batch's final_decode (+ _min_res), final_extract and guidance_decode (+ _min_res),
        # and "dense" (default) | "sparse", the extractor of the guidance loop's exact-size path (guidance_extract_mode)
        opts = _schedule_options(self.vae, guid_res, final_res, *[kwargs.pop(k, None) for k in _OPTION_KWARGS])
        guid_sparse = guidance_extract_mode(kwargs.pop("guidance_extract", None)) == "sparse"
        J_regressor = kwargs.pop("J_regressor", None)                        # default: the file of PL:1218
        on_phase_end = kwargs.pop("on_phase_end", None)      # hook(phase, denoising step, GuidanceBatch): inspection / tests
        self.stats = stats = {"inner_iterations": 0, "skipped_empty": 0}
        if opts.guid_band:
            stats["guidance_decode"] = {}
        if guid_sparse:
            stats["guidance_extract"] = {"calls": 0, "cubes": 0, "vertices": 0, "faces": 0}
        self.loss_log = loss_log = []        # (phase, denoising step, iteration, loss terms) every 10th iteration, like the prints
        self.param_log = param_log = []      # (phase, denoising step, the 16 similarity parameters, noise prediction) at phase end
        device, dtype = self.device, self.dtype
        cfg0 = config() if config is not None else E.OptimizationConfig()

        debug_root = os.environ.get("FOHO_DEBUG_DIR")
        index = cropped_obj_img_path.split("/")[-1].split("_")[0]
        log = None
        if debug_root:
            save_dir = os.path.join(debug_root, f"{datetime.datetime.now().strftime('%Y%m%d_%H%M%S')}_exp_obj{index}_inpainted")
            os.makedirs(save_dir, exist_ok=True)
            log = open(os.path.join(save_dir, "losses.txt"), "w")

        def say(msg):
            if log:
                log.write(msg + "\n")
            print(msg)

        num_inference_steps = cfg0.num_inference_steps
        handopt_start_step = cfg0.handopt_start_step
        guidance_end_step = num_inference_steps
        if debug_root:
            keys = ["obj_guidance_scale", "optimization_steps_hand", "optimization_steps_joint", "optimization_steps_scale",
                    "num_inference_steps", "guidance_start_step", "handopt_start_step", "phase1_hand_lrs", "phase2_hand_lrs",
                    "obj_lrs", "obj_2half_lrs", "noise_obj_lr1", "noise_obj_lr2", "use_intersection_loss"]
            with open(os.path.join(save_dir, "params.json"), "w") as f:
                json.dump({**{k: getattr(cfg0, k) for k in keys}, "guidance_end_step": guidance_end_step}, f, indent=4)

        sch = self._schedule_setup(image, guidance_scale, cfg0.batch_size, num_inference_steps, guid_res, sigmas=sigmas)
        xyz_samples, bmin, bmax = sch.xyz, sch.bmin, sch.bmax
        obj_latents = self.prepare_latents(cfg0.batch_size, dtype, device, generator).clone()

        fov = float(renderer.rasterizer.cameras.fov) if renderer is not None else None
        paths = dict(hand_mask_path=hand_mask_path, obj_mask_path=obj_mask_path, moge_mesh_path=moge_mesh_path, h2m_rt_path=h2m_rt_path,
                     aligned_mano_mesh_path=aligned_mano_mesh_path, hamer_for_guid_path=hamer_for_guid_path)
        (scene,), (T_h2m,), (hand_moge,), (hand_faces,) = _load_scenes([paths], [fov], J_regressor, device)
        gb = E.GuidanceBatch([scene], device=device, grid_res=guid_res, n_renders=2)
        hip_dec = getattr(self.vae, "hip_geo", None)
        decoder = _StepDecoder(self.vae, sch, opts, guid_res, final_res, stats, num_chunks)

        # Phases B and C re-extract the object from the latent in every iteration (PL:1391-1393, 1507-1509): vertex count,
        # face count and connectivity change each time.  Fast path: engine.SdfObjective -- iso-surfacing, installing the new
        # object, the fused step and the backward to the SDF as one hipGraph replay over capacity-sized buffers, the counts
        # staying on the device.  Iterations it cannot serve (capacity exceeded, a surface that is not a closed manifold)
        # are redone on the exact-size path (ops.flexicubes + GuidanceBatch.objective), which handles any mesh.
        fast = {"gb": None, "obj": None, "cap": (0, 0)}

        def fast_objective(cap):
            if fast["gb"] is None or fast["cap"] != cap:
                g2 = E.GuidanceBatch([scene], device=device, grid_res=guid_res, n_renders=2, obj_capacity=cap)
                fast.update(gb=g2, obj=E.SdfObjective(g2, xyz_samples, guid_res), cap=cap)
            return fast["gb"], fast["obj"]

        def sync_state(src, dst):       # pose parameters and optimiser moments travel with the iteration
            for name in ("params", "adam_m", "adam_v", "adam_t", "flags"):
                getattr(dst, name).copy_(getattr(src, name))

        def phase_ended(phase, i, noise_pred):
            param_log.append((phase, i, gb.params[0].detach().clone(), noise_pred))
            if on_phase_end is not None:
                on_phase_end(phase, i, gb)

        def hand_phase(i):
            """Phase A with the reference's prints (PL:1351-1355) and, under FOHO_DEBUG_DIR, its plots of the rendered hand normals every 10
            iterations (PL:1331-1333)."""
            n = int(cfg0.optimization_steps_hand)
            cfg_eval, _ = E.phase_cfg("A", cfg0, denoise_i=i, do_update=False)
            plots = bool(debug_root) and n % 10 == 0

            def first_losses():       # the k = 0 losses the reference prints: one evaluation at the current parameters, no update
                gb.step(cfg_eval)
                l0 = gb.loss_dict(0)
                loss_log.append(("A", i, 0, l0))
                say(f"Opt step 0, loss_2d_kps: {l0['kps']}, loss_normal_hand: {l0['normal0']}, loss_disp_hand: {l0['disp0']}")

            def plot(rep):            # the render iteration k = 10 rep starts from
                gb.step(cfg_eval)
                E.save_grid(E.normal_map(gb, E.L.FACES_HAND), scene["moge_normal"], os.path.join(save_dir, f"rendered_normal_hand_t{i}_opt{10 * rep}.png"))

            flags = _hand_phase(gb, cfg0, i, stats, device, spg=10 if plots else None, after_capture=first_losses,
                                before_replay=plot if plots else None)
            # the reference has no NaN guard in phase A (PL:1320-1358): a NaN loss there poisons the hand pose;
            # here the sticky flag freezes the parameters instead -- say so rather than continue silently
            if int(flags[0]) & 1:
                say("Total loss is NaN in the hand-only phase: hand parameters frozen at their last finite value")
            l = gb.loss_dict(0)
            say(f"Opt step {n - 1}, loss_2d_kps: {l.get('kps', 0.0)}, total: {l['total']}")
            phase_ended("A", i, None)

        def latent_phase(phase, iters, i, t, noise_pred, lr, nan_returns_none):
            """Phases B / C (PL:1362-1453 / 1456-1601): `iters` iterations of decode -> fused step -> AdamW."""
            cfg, n_renders = E.phase_cfg(phase, cfg0, denoise_i=i, do_update=True)
            gb.set_n_renders(n_renders)
            gb.reset_optimizer()
            noise_pred = noise_pred.clone().detach().requires_grad_(True)
            opt = torch.optim.AdamW([{"params": [noise_pred], "lr": lr}], eps=1e-4)
            use_fast = os.environ.get("FOHO_EXACT_SIZE_OBJECTIVE") != "1"
            cap = fast["cap"] if fast["cap"][0] else (8 * guid_res * guid_res, 16 * guid_res * guid_res)
            if not fast["cap"][0] and os.environ.get("FOHO_OBJ_CAPACITY"):      # "verts,faces": start value (tests: force the growth path)
                cap = tuple(int(x) for x in os.environ["FOHO_OBJ_CAPACITY"].split(","))
            for k in range(int(iters)):
                opt.zero_grad()
                sdf = decoder.guidance(self.scheduler.step_final(noise_pred, t, obj_latents))[0]
                loss, cur = None, gb
                if use_fast:
                    g2, fobj = fast_objective(cap)
                    g2.set_n_renders(n_renders)
                    sync_state(gb, g2)
                    loss = fobj(sdf, cfg)
                    nv, nf, fl = fobj.status()[0]          # one read-back per iteration (the reference's NaN test is one, too)
                    if hip_dec is not None:
                        _bound_active_rows(self.vae, fobj.active_rows()[0])
                    if fl & 64:                            # empty iso-surface (PL:1394-1397, 1511-1513)
                        print("Invalid mesh detected, aborting step!")
                        stats["skipped_empty"] += 1
                        continue
                    if fl & 16:                            # larger than the capacity: grow it, this iteration goes the exact way
                        cap = (max(cap[0], 2 * nv), max(cap[1], 2 * nf))
                        stats["capacity_grown"] = stats.get("capacity_grown", 0) + 1
                    if fl & 48:
                        loss = None
                    else:
                        cur = g2
                if loss is None:
                    if guid_sparse:      # the same mesh from axis tables; two host reads, so not for capacity mode's graph
                        verts, faces, _, est = ops.flexicubes_sparse_grad(ops.grid_axes(bmin, bmax, guid_res), sdf, guid_res, return_stats=True)
                    else:
                        verts, faces, _ = ops.flexicubes(xyz_samples, sdf, guid_res)
                    if verts.shape[0] == 0:
                        print("Invalid mesh detected, aborting step!")
                        stats["skipped_empty"] += 1
                        continue
                    _bound_active_rows(self.vae, xyz_samples.shape[0])     # the exact-size path: no count known before the backward -- all rows
                    loss = gb.objective(verts, faces, cfg)
                    stats["exact_size_iterations"] = stats.get("exact_size_iterations", 0) + 1
                    if guid_sparse:      # tallied with the iterations the extraction served
                        stats["guidance_extract"]["calls"] += 1
                        for key in ("cubes", "vertices", "faces"):
                            stats["guidance_extract"][key] += est[key]
                stats["inner_iterations"] += 1
                if torch.isnan(loss):
                    print("Total loss is NaN")
                    if cur is not gb:
                        sync_state(cur, gb)
                    if nan_returns_none:
                        return None
                    break
                if k % 10 == 0:
                    if debug_root and phase == "B":     # PL:1417-1419
                        E.save_grid(E.normal_map(cur, E.L.FACES_OBJ), scene["moge_normal"] * np.asarray(scene["obj_mask"], np.float32)[..., None],
                                    os.path.join(save_dir, f"rendered_obj_normal_t{i}_opt{k}.png"))
                    l = cur.loss_dict(0)
                    loss_log.append((phase, i, k, l))
                    say(f"Opt step {k}, object loss: {l['edge']}, loss_intersection: {l.get('intersection', 0.0)}, "
                        f"total: {l['total']}")
                loss.backward()
                opt.step()
                if cur is not gb:
                    sync_state(cur, gb)
            gb.raise_on_flags(strict_k=False)
            _check_rows_dropped(hip_dec)
            phase_ended(phase, i, noise_pred.detach().clone())
            return noise_pred.detach().clone()

        obj_out = hand_out = None
        for i, t in enumerate(sch.timesteps):
            noise_pred_obj = self._noise_prediction(sch, obj_latents, i, t, cfg0)
            if i >= handopt_start_step:
                with torch.enable_grad():
                    if i == handopt_start_step:
                        say(f"Pre-guidance step {i}, optimizing hands only")
                        hand_phase(i)
                    elif i <= guidance_end_step:
                        with _latent_phase_scope(hip_dec):
                            if i == handopt_start_step + 1:              # phase B: object transform + latent (PL:1361-1453)
                                say(f"Object optimization step {i}, optimizing object transformation")
                                noise_pred_obj = latent_phase("B", cfg0.optimization_steps_scale, i, t, noise_pred_obj, cfg0.noise_obj_lr1,
                                                              nan_returns_none=True)
                            else:                                        # phase C: joint (PL:1455-1601)
                                say(f"Joint optimization step {i}, optimizing hands and object together")
                                noise_pred_obj = latent_phase("C", cfg0.optimization_steps_joint, i, t, noise_pred_obj, cfg0.noise_obj_lr2,
                                                              nan_returns_none=False)
                        if noise_pred_obj is None:
                            return None
                noise_pred_obj = noise_pred_obj.detach().clone()

            obj_latents = self.scheduler.step(noise_pred_obj, t, obj_latents).prev_sample

            # current clean-sample estimate as a mesh in the MoGe world (PL:1612-1661); the last one is the result
            last = i == num_inference_steps - 1
            res, xyz, extract = decoder.step_grid(last)
            sdf = decoder.step(self.scheduler.step_final(noise_pred_obj, t, obj_latents), last, res, xyz)
            obj_now, hand_now = _meshes_in_moge_world(*extract(sdf[0], 0), T_h2m, gb.params[0], hand_moge, hand_faces, i >= handopt_start_step)
            hand_out = hand_out if hand_now is None else hand_now
            if obj_now is None:
                continue
            obj_out = obj_now
            obj_world, faces = obj_out.verts_packed(), obj_out.faces_packed()
            if debug_root:      # PL:1664-1667: the scene of this denoising step against the MoGe normals
                if hand_now is not None:
                    dv = torch.cat([hand_now.verts_packed(), obj_world], 0)
                    df = torch.cat([hand_faces, faces + hand_now.verts_packed().shape[0]], 0)
                else:
                    dv, df = obj_world, faces
                dn, _, _ = E.hip_render_fn(device)(dv.detach().cpu().numpy(), df.cpu().numpy(), gb.H, gb.W, scene["fov"])
                E.save_grid(dn, scene["moge_normal"], os.path.join(save_dir, f"rendered_normal_t{i}.png"))
            if debug_root and i in (14, num_inference_steps - 1):
                from . import meshio
                tag = "final" if last else f"guidance_step_{i}"
                meshio.save_ply(os.path.join(save_dir, f"{tag}_hand_mesh.ply"), hand_out.verts_packed().cpu().numpy(),
                                hand_faces.cpu().numpy())
                meshio.save_ply(os.path.join(save_dir, f"{tag}_obj_mesh.ply"), obj_world.cpu().numpy(), faces.cpu().numpy())
        if log:
            log.close()
        self.guidance_batch = gb
        return obj_out, hand_out
