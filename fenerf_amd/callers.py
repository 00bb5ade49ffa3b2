"""Thin callers of the generator API -- the library-level counterparts of the reference's inference scripts
(SURVEY §8f.2 / f.3).  They add nothing to the hot path: every render goes through generator.staged_forward* /
siren.forward_with_frequencies_phase_shifts, i.e. the HIP kernels.

reference: mask2color + COLOR_MAP  train_double_latent_semantic.py:35-72
           multi-view loop         render_multiview_images_double_semantic.py:24-85
           voxel-grid evaluation   extract_double_semantic_shapes.py:13-90
           inversion loop          inverse_render_double_semantic.py:306-410
           latent interpolation    render_video_interpolation_semantic.py:131-187
"""
import numpy as np
import torch

from . import native

# label id -> RGB (train_double_latent_semantic.py:35-55); configuration data of the dataset's 19 classes
COLOR_MAP = {
    0: [0, 0, 0], 1: [204, 0, 0], 2: [76, 153, 0], 3: [204, 204, 0], 4: [51, 51, 255], 5: [204, 0, 204], 6: [0, 255, 255],
    7: [255, 204, 204], 8: [102, 51, 0], 9: [255, 0, 0], 10: [102, 204, 0], 11: [255, 255, 0], 12: [0, 0, 153],
    13: [0, 0, 204], 14: [255, 51, 153], 15: [0, 204, 204], 16: [0, 51, 0], 17: [255, 153, 51], 18: [0, 204, 0],
}
_COLOR_LUT = np.zeros((max(COLOR_MAP) + 1, 3), dtype=np.float32)
for _k, _v in COLOR_MAP.items():
    _COLOR_LUT[_k] = _v


def mask2color(masks, device=None, scale=None):
    """[B,19,H,W] logits -> [B,3,H,W] float colours (0..255) on the CPU, like the reference: argmax over the label
    channels (first index wins ties) then the LUT (train_double_latent_semantic.py:66-72)."""
    # the label channels of an image that is already on the host (staged_forward's result) go through numpy: single-threaded, 4 ms per
    # 256 x 256 image wherever it runs -- torch's CPU argmax over a non-last dimension takes 9 ms with a sane thread count and 50-70 ms in
    # a container whose CPU quota is far below its logical CPU count (the GPU boxes of this project: 256 logical CPUs, 16 granted), which
    # made it the largest item of a 256 x 256 multi-view render (tools/exp/callers_timing.py).  numpy's argmax also returns the first maximum.
    # `device`: a GPU the caller has at hand -- the host image's label channels take the argmax there (0.5 ms round trip through pinned memory
    # instead of 4 ms; the device's argmax also returns the first maximum, NaNs included: tools/exp/argmax_ties_probe.py)
    if not masks.is_cuda and device is not None and torch.device(device).type == "cuda":
        masks = masks.to(device, non_blocking=True)
    if masks.is_cuda:
        idx = native.to_host(torch.argmax(masks, dim=1).to(torch.uint8)).numpy()
    else:
        idx = np.argmax(masks.detach().numpy(), axis=1)
    out = np.ascontiguousarray(_COLOR_LUT[idx].transpose(0, 3, 1, 2))
    if scale is not None:          # `mask2color(...) / 255.` of the reference's scripts, as one fp32 division per element here (numpy) instead of
        out = out / np.float32(scale)    # a torch CPU operation per view (5-15 ms each where the CPU quota is far below the CPU count)
    return torch.from_numpy(out)


def multiview_kwargs(curriculum, image_size=256, ray_step_multiplier=2, lock_view_dependence=False):
    """The kwargs bag render_multiview_images_double_semantic.py:43-54 builds from a curriculum."""
    c = dict(curriculum)
    c["num_steps"] = curriculum[0]["num_steps"] * ray_step_multiplier
    c["img_size"] = image_size
    c["psi"] = 0.7
    c["v_stddev"] = 0
    c["h_stddev"] = 0
    c["lock_view_dependence"] = lock_view_dependence
    c["last_back"] = False
    c["nerf_noise"] = 0
    return {k: v for k, v in c.items() if type(k) is str}


def load_generator(path, device, use_ema=True, reset_render_options=True):
    """What every inference script of the reference does first (render_multiview_images_double_semantic.py:58-66,
    render_video_interpolation_semantic.py:317-324): unpickle the generator module saved by the training loop
    (`torch.save(generator_ddp.module, 'generator.pth')`, train...py:524), unpickle the torch_ema object next to it
    (`<prefix>ema.pth`, the prefix being everything before 'generator' in the path) and copy the averaged weights in, then
    set_device + eval.  Pickles written by the reference resolve through compat.install_aliases(): its module paths
    (generators.generators.*, siren.siren.*) map to this package and torch_ema.ema.ExponentialMovingAverage to fenerf_amd.ema
    when torch_ema is not installed (same attribute layout: decay, num_updates, shadow_params, collected_params).
    `reset_render_options`: the multi-view and inversion scripts overwrite three attributes of the pickled module
    (softmax_label = False, neural_renderer_img / _seg = None; render_multiview...:60-62, inverse_render...), the video script keeps
    what the pickle says (render_video_interpolation_semantic.py:317-324) -- its front end passes False.  `use_ema=False` (the tools'
    --no_ema) renders the raw generator weights; the reference has no such switch and fails without the ema file."""
    import os
    from . import compat
    compat.install_aliases()
    device = torch.device(device)
    generator = torch.load(path, map_location=device, weights_only=False)
    if reset_render_options:
        generator.softmax_label = False
        generator.neural_renderer_img = None
        generator.neural_renderer_seg = None
    ema_file = path.split("generator")[0] + "ema.pth"
    if use_ema:
        if not os.path.exists(ema_file):
            raise FileNotFoundError(f"{ema_file}: the reference loads the EMA weights next to the generator pickle")
        ema = torch.load(ema_file, map_location=device, weights_only=False)
        ema.copy_to(generator.parameters())
    generator.set_device(device)
    generator.eval()
    return generator


# what a Camera replaces in a kwargs bag written for the angle camera
_ANGLE_CAMERA_KEYS = ("img_size", "fov", "h_mean", "v_mean", "h_stddev", "v_stddev", "sample_dist")


def _latent_dims(generator, default=256):
    """(z_geo_dim, z_app_dim): the reference hard-codes 256 (render_multiview...:79-80); read from the module when it says otherwise."""
    return int(getattr(generator, "z_geo_dim", default)), int(getattr(generator, "z_app_dim", default))


def render_multiview(generator, curriculum, seed, device, face_angles=(-0.5, -0.25, 0.0, 0.25, 0.5), image_size=256,
                     ray_step_multiplier=2, lock_view_dependence=False, z_dim=None, latents=None, baked=None, geometry=False, labels_only=False,
                     proposal=None, cameras=None):
    """Five yaw angles of one identity (render_multiview_images_double_semantic.py:66-85).
    -> (images [V,3,S,S] in [-1,1], segmaps [V,3,S,S] in [0,1]) on the CPU.
    geometry: True, or a dict of render_geometry's options (light, ambient, background, alpha_min, space) -- every view goes through
    render_geometry (the same render) and the result gains (normals [V,3,S,S] in [-1,1], shaded [V,1,S,S]).
    latents: optional (z_geo, z_app) instead of the seeded draws (tests teacher-force the reference's CPU-generator values).
    baked: a lattice resolution -- the identity is baked once (bake_field, view direction locked) and every view is rendered from the
    lattice by BakedField.render with the exact route's rays and draws: an approximation.  None = the exact renders.
    labels_only: only the semantic row and the depth, through generator.staged_geometry (no colour branch where the model's density route
    serves it) -> (segmaps [V,3,S,S] in [0,1] -- the default call's, bit for bit --, depth maps [V,S,S]); not with baked or geometry.
    proposal: a lattice resolution -- the identity's DENSITY is baked once (bake_density) and every view places its samples from the
    lattice and evaluates the network there (DensityField.render: one SIREN pass, view-dependent colour kept).  Not
    with baked, geometry or labels_only.  None = the exact renders.
    cameras: a list of fenerf_amd.camera.Camera (one image each, frames of one size) -- the views are theirs instead of the five yaw angles
    (generator.staged_forward_camera: roll, distance, a window of the image; image_size and face_angles are then not read).  The exact
    colour renders only: not with baked, geometry, labels_only or proposal."""
    _refuse_proposal_with("render_multiview", proposal, baked=baked, geometry=geometry, labels_only=labels_only)
    if cameras is not None and (baked is not None or geometry or labels_only or proposal is not None):
        raise ValueError("render_multiview: cameras take the exact colour renders; none of baked, geometry, labels_only, proposal")
    if cameras is not None and len(cameras) == 0:
        raise ValueError("render_multiview: cameras is an empty list (None = the five yaw angles)")
    if labels_only and (baked is not None or geometry):
        raise ValueError("render_multiview: labels_only renders the exact semantic row; it takes neither baked nor geometry")
    kw = multiview_kwargs(curriculum, image_size, ray_step_multiplier, lock_view_dependence)
    h_mean = kw["h_mean"]
    zg_dim, za_dim = (z_dim, z_dim) if z_dim is not None else _latent_dims(generator)
    images, segmaps, normals, shadeds, depths = [], [], [], [], []
    geo = dict(geometry) if isinstance(geometry, dict) else {}
    field = None
    for a in (face_angles if cameras is None else cameras):
        if cameras is None:
            kw["h_mean"] = a + h_mean
        torch.manual_seed(seed)
        z_geo = torch.randn((1, zg_dim), device=device)
        z_app = torch.randn((1, za_dim), device=device)
        if latents is not None:
            z_geo, z_app = (torch.as_tensor(t, dtype=torch.float32, device=device) for t in latents)
        with torch.no_grad():
            if cameras is not None:
                img, _ = generator.staged_forward_camera(z_geo, z_app, a, **{k: v for k, v in kw.items() if k not in _ANGLE_CAMERA_KEYS})
                images.append(img[:, -3:])
                segmaps.append(mask2color(img[:, :-3], device, scale=255.0))
                continue
            if labels_only:
                seg, depth = generator.staged_geometry(z_geo, z_app, **kw)
                segmaps.append(mask2color(seg, device, scale=255.0))
                depths.append(depth)
                continue
            if proposal is not None:
                avg = generator.generate_avg_frequencies()          # staged_forward's draws before its render, per view
                if field is None:
                    field = _proposal_multiview_field(generator, z_geo, z_app, avg, kw, proposal)
                img, _, _ = field.render(generator, **kw)
            elif baked is None and not geometry:
                img, _ = generator.staged_forward(z_geo, z_app, **kw)
            elif baked is None:
                view = render_geometry(generator, z_geo, z_app, **geo, **kw)
            else:
                avg = generator.generate_avg_frequencies()          # staged_forward's draws before its render, per view
                if field is None:
                    field = _baked_multiview_field(generator, z_geo, z_app, avg, kw, baked)
                if geometry:
                    view = field.render_geometry(generator, **geo, **kw)
                else:
                    img, _, _ = field.render(generator, **kw)
        if geometry:
            img = view["pixels"]
            normals.append(view["normal"])
            shadeds.append(view["shaded"])
        images.append(img[:, -3:])
        segmaps.append(mask2color(img[:, :-3], device, scale=255.0))
    if labels_only:
        return torch.cat(segmaps), torch.cat(depths)
    if geometry:
        return torch.cat(images), torch.cat(segmaps), torch.cat(normals), torch.cat(shadeds)
    return torch.cat(images), torch.cat(segmaps)


def create_samples(N=256, voxel_origin=(0, 0, 0), cube_length=2.0, device=None):
    """Voxel-centre coordinates [1, N^3, 3] exactly as the reference builds them (extract_double_semantic_shapes.py:13-35):
    note the y / x indices are (i / N) % N and (i / N / N) % N in FLOAT arithmetic (not floor-divided) -- kept as is.
    device: build them there (the same statements: int64 -> float conversion, IEEE division (by a tensor divisor), fmod, one multiply and one add per coordinate
    -- bit for bit the host's values, a GPU test compares) instead of on the host followed by a 200-MB pageable copy at N = 256."""
    voxel_origin = np.array(voxel_origin) - cube_length / 2
    voxel_size = cube_length / (N - 1)
    overall_index = torch.arange(0, N ** 3, 1, dtype=torch.long, device=device)
    samples = torch.zeros(N ** 3, 3, device=device)
    # (on a GPU torch divides by a Python scalar as a multiplication by its reciprocal -- not the host's correctly rounded quotient unless N
    # is a power of two; a tensor divisor takes the IEEE division: tools/exp/div_probe.py)
    Nf = N if samples.device.type == "cpu" else torch.tensor(float(N), device=samples.device)
    samples[:, 2] = overall_index % N
    samples[:, 1] = (overall_index.float() / Nf) % Nf
    samples[:, 0] = ((overall_index.float() / Nf) / Nf) % Nf
    samples[:, 0] = (samples[:, 0] * voxel_size) + voxel_origin[2]
    samples[:, 1] = (samples[:, 1] * voxel_size) + voxel_origin[1]
    samples[:, 2] = (samples[:, 2] * voxel_size) + voxel_origin[0]
    return samples.unsqueeze(0), voxel_origin, voxel_size


def _lattice_sigma(nat, samples, fg, pg, fa, pa, want_labels=False):
    """sigma [1,P] of the lattice points (view direction locked) and, with want_labels, the argmax label [1,P] uint8 (first maximum wins,
    torch.argmax on the label logits).  The density route where the model serves it (NativeModel.supports_density: no colour branch,
    one float per point, nothing to slice), else the full forward -- the same bits either way."""
    if nat.supports_density():
        if want_labels and nat.n_labels() > 0:
            rows = nat.siren_density(samples, fg, pg, labels=True)
            return rows[..., -1], torch.argmax(rows[..., :-1], dim=-1).to(torch.uint8)
        sigma = nat.siren_density(samples, fg, pg, labels=False)
        return sigma, (torch.zeros_like(sigma, dtype=torch.uint8) if want_labels else None)
    out = nat.siren_forward(samples, None, fg, pg, fa, pa)          # None = locked view dir
    labels = None
    if want_labels:
        labels = torch.argmax(out[..., :-4], dim=-1).to(torch.uint8) if out.shape[-1] > 4 else torch.zeros(out.shape[:-1], dtype=torch.uint8, device=out.device)
    return out[..., -1], labels


def sample_generator(generator, z_geo, z_app=None, max_batch=None, voxel_resolution=256, voxel_origin=(0, 0, 0), cube_length=2.0,
                     psi=0.5, return_labels=False):
    """Density volume [N,N,N] (numpy) of one identity for marching cubes (extract_double_semantic_shapes.py:38-62):
    truncated FiLM parameters, view direction locked to (0,0,-1).  One fused kernel launch evaluates all N^3 points;
    `max_batch` is accepted for signature compatibility and ignored.  (The reference passes the same z to both mapping
    networks; pass z_app to differ.)  return_labels: -> (density volume, label volume [N,N,N] uint8: the argmax of every point's label
    logits, first maximum wins)."""
    z_app = z_geo if z_app is None else z_app
    N = voxel_resolution
    samples, _, _ = create_samples(voxel_resolution, voxel_origin, cube_length, device=z_geo.device)
    avg_fg, avg_pg, avg_fa, avg_pa = generator.generate_avg_frequencies()
    with torch.no_grad():
        raw_fg, raw_pg = generator.siren.geo_mapping_network(z_geo)
        raw_fa, raw_pa = generator.siren.app_mapping_network(z_app)
        fg, pg = avg_fg + psi * (raw_fg - avg_fg), avg_pg + psi * (raw_pg - avg_pg)
        fa, pa = avg_fa + psi * (raw_fa - avg_fa), avg_pa + psi * (raw_pa - avg_pa)
        sigma, labels = _lattice_sigma(generator.siren.native(samples.device), samples, fg, pg, fa, pa, want_labels=return_labels)
    volume = native.to_host(sigma.reshape(N, N, N).contiguous()).numpy()
    if return_labels:
        return volume, native.to_host(labels.reshape(N, N, N).contiguous()).numpy()
    return volume


def film_from_inversion(meta, device=None):
    """(freq_geo, freq_app, phase_geo, phase_app) = mean + offset of an inversion checkpoint (the dict inverse_render returns / the
    reference's `freq_phase_offset_<name>.pth`), in forward_with_frequencies' argument order (extract_double_semantic_shapes.py:127-133,
    inverse_render_double_semantic.py:465-467)."""
    t = (lambda v: v.detach().to(device)) if device is not None else (lambda v: v.detach())
    return (t(meta["w_geo_frequencies"]) + t(meta["w_geo_frequency_offsets"]), t(meta["w_app_frequencies"]) + t(meta["w_app_frequency_offsets"]),
            t(meta["w_geo_phase_shifts"]) + t(meta["w_geo_phase_shift_offsets"]), t(meta["w_app_phase_shifts"]) + t(meta["w_app_phase_shift_offsets"]))


def sample_generator_wth_frequencies_phase_shifts(generator, meta, max_batch=None, voxel_resolution=256, voxel_origin=(0, 0, 0),
                                                  cube_length=2.0, psi=0.5, return_labels=False):
    """Density volume [N,N,N] of an INVERTED identity (extract_double_semantic_shapes.py:65-87, the reference's spelling of the name):
    meta carries 'truncated_frequencies_geo' / '_app' and 'truncated_phase_shifts_geo' / '_app' (the script fills them with mean +
    offset of an inversion checkpoint, :127-133 -- film_from_inversion above); view direction locked to (0, 0, -1); `max_batch` and `psi`
    are accepted and ignored (the reference ignores psi here too).  return_labels: as sample_generator's."""
    samples, _, _ = create_samples(voxel_resolution, voxel_origin, cube_length, device=generator.device)
    with torch.no_grad():
        sigma, labels = _lattice_sigma(generator.siren.native(samples.device), samples, meta["truncated_frequencies_geo"], meta["truncated_phase_shifts_geo"],
                                       meta["truncated_frequencies_app"], meta["truncated_phase_shifts_app"], want_labels=return_labels)
    shape = (voxel_resolution,) * 3
    volume = native.to_host(sigma.reshape(shape).contiguous()).numpy()
    if return_labels:
        return volume, native.to_host(labels.reshape(shape).contiguous()).numpy()
    return volume


MESH_NORMAL_CHUNK = 262144       # vertices per differentiable SIREN call of extract_mesh's normals: bounds the tape


def extract_mesh(generator, z_geo, z_app=None, *, film=None, voxel_resolution=256, voxel_origin=(0, 0, 0), cube_length=2.0, psi=0.5, iso=10.0,
                 attributes=("normal", "label", "rgb"), keep="all", simplify=None):
    """Labelled, coloured iso-surface of one identity: the step the reference leaves to skimage.measure.marching_cubes + plyfile
    (extract_shapes.py, extract_double_semantic_shapes.py).  The lattice is evaluated exactly as sample_generator does (truncated FiLM
    parameters, locked view direction, one fused launch) -- or, with film= (the meta dict of
    sample_generator_wth_frequencies_phase_shifts), as that function does; z_geo / z_app / psi are then ignored.  The density volume stays on
    the device and goes through native.mesh_from_volume (marching tetrahedra, include/fenerf.h) with the per-column origin and spacing of
    create_samples: vertex column k is in the coordinates of samples[:, k], so vertices can be fed straight back to the SIREN.  That is what
    happens next: one forward at the vertices (padded to whole 32-point tiles) gives `label` (argmax of the label logits, uint8) and `rgb`
    (the SIREN's rgb as the image writer maps a pixel: * 2 - 1, then [-1, 1] -> 0..255); `normal` is -grad(sigma) normalised, through the
    differentiable bare-SIREN route in chunks of at most MESH_NORMAL_CHUNK vertices.
    -> dict of numpy arrays: vertices [V,3] float32, faces [F,3] int32 and the requested attributes (normal [V,3] float32, label [V] uint8,
    rgb [V,3] uint8).  iso = 10.0 is this project's choice: the reference's scripts name no level.
    keep = "largest" | a number of lattice points: detached blobs of density go before meshing -- only the largest connected component of
    {sigma >= iso}, or every component of at least that many points, stays (native.filter_volume); the dict gains `components`, the count
    before filtering.  simplify = an integer factor >= 2: the vertices of every factor^3 block of cells merge into their mean
    (native.cluster_mesh) after meshing and before the attribute pass, so label, rgb and normal are evaluated at the vertices that survive
    (a merged vertex lies near the surface, not on it).  With the defaults neither runs.
    Like sample_generator, the z_geo route calls generate_avg_frequencies, whose 2 x 10,000 draws start from the generator state the caller
    leaves: for the surface of a volume sample_generator returned, restore that state first (tools/extract_shapes.py re-seeds)."""
    from . import imageio_lite
    unknown = set(attributes) - {"normal", "label", "rgb"}
    if unknown:
        raise ValueError(f"extract_mesh: unknown attributes {sorted(unknown)}")
    if not (keep in ("all", "largest") or (isinstance(keep, int) and not isinstance(keep, bool) and keep >= 1)):
        raise ValueError(f'extract_mesh: keep is "all", "largest" or a number of points >= 1, not {keep!r}')
    if not (simplify is None or (isinstance(simplify, int) and not isinstance(simplify, bool) and simplify >= 2)):
        raise ValueError(f"extract_mesh: simplify is None or an integer factor >= 2, not {simplify!r}")
    N = voxel_resolution
    siren = generator.siren
    with torch.no_grad():
        if film is None:
            z_app = z_geo if z_app is None else z_app
            device = z_geo.device
            avg_fg, avg_pg, avg_fa, avg_pa = generator.generate_avg_frequencies()
            raw_fg, raw_pg = siren.geo_mapping_network(z_geo)
            raw_fa, raw_pa = siren.app_mapping_network(z_app)
            fg, pg = avg_fg + psi * (raw_fg - avg_fg), avg_pg + psi * (raw_pg - avg_pg)
            fa, pa = avg_fa + psi * (raw_fa - avg_fa), avg_pa + psi * (raw_pa - avg_pa)
        else:
            device = generator.device
            fg, pg = film["truncated_frequencies_geo"], film["truncated_phase_shifts_geo"]
            fa, pa = film["truncated_frequencies_app"], film["truncated_phase_shifts_app"]
        samples, origin, voxel_size = create_samples(N, voxel_origin, cube_length, device=device)
        nat = siren.native(samples.device)
        sigma = _lattice_sigma(nat, samples, fg, pg, fa, pa)[0].reshape(N, N, N).contiguous()
        components = None
        if keep != "all":
            sigma, stats = native.filter_volume(sigma, iso, keep, out=sigma)
            components = int(native.to_host(stats)[1])
        # samples[:, k] = (lattice index along axis k) * voxel_size + origin[2 - k]  (create_samples)
        frame = dict(origin=(origin[2], origin[1], origin[0]), spacing=(voxel_size,) * 3)
        vertices, faces = native.mesh_from_volume(sigma, iso, **frame)
        if simplify is not None:
            vertices, faces = native.cluster_mesh(vertices, faces, shape=(N, N, N), factor=simplify, **frame)
        V = vertices.shape[0]
        mesh = dict(vertices=native.to_host(vertices).numpy(), faces=native.to_host(faces).numpy())
        if components is not None:
            mesh["components"] = components
        if V and ("label" in attributes or "rgb" in attributes):
            pad = (-V) % 32
            pts = torch.cat([vertices, vertices[-1:].expand(pad, -1)])[None] if pad else vertices[None]
            rows = nat.siren_forward(pts.contiguous(), None, fg, pg, fa, pa)[0, :V]
            if "label" in attributes:
                mesh["label"] = native.to_host(torch.argmax(rows[:, :-4], dim=1).to(torch.uint8)).numpy()
            if "rgb" in attributes:
                pix = native.to_host((rows[:, -4:-1] * 2 - 1).t().contiguous()).numpy()[None, :, :, None]        # [1, 3, V, 1]: an image one pixel wide
                mesh["rgb"] = imageio_lite.to_uint8_hwc(imageio_lite._grid_np(pix, normalize=True, value_range=(-1, 1)))[:, 0]
        elif not V:
            mesh.update({k: np.zeros(s, d) for k, s, d in (("label", (0,), np.uint8), ("rgb", (0, 3), np.uint8)) if k in attributes})
    if "normal" in attributes:
        g = _sigma_input_grads(siren, vertices[None], fg, pg, fa, pa, MESH_NORMAL_CHUNK)[0]
        normal = -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        mesh["normal"] = native.to_host(normal).numpy()
    return mesh


def _sigma_input_grads(siren, points, fg, pg, fa, pa, chunk):
    """d sigma / d position at points [B,P,3] on the device -> [B,P,3], through the differentiable bare-SIREN route (forward-save, chain,
    input-gradient pass; locked view direction) in chunks of at most `chunk` points per image"""
    from .siren import autograd as siren_autograd
    grads = torch.empty(tuple(points.shape), dtype=torch.float32, device=points.device)
    # only the positions take a gradient: with every weight constant the backward is the chain and the input-gradient pass alone
    params = [p for p in siren._render_params() if p.requires_grad]
    for p in params:
        p.requires_grad_(False)
    try:
        for s0 in range(0, points.shape[1], chunk):
            with torch.enable_grad():
                pts = points[:, s0:s0 + chunk].detach().clone().requires_grad_(True)
                sig = siren_autograd.siren_apply(siren, pts, None, fg.detach(), pg.detach(), fa.detach(), pa.detach())[..., -1]
                g, = torch.autograd.grad(sig.sum(), pts)
            grads[:, s0:s0 + chunk] = g
    finally:
        for p in params:
            p.requires_grad_(True)
    return grads


# ---- many views of one identity: bake the field into a lattice once, render every view by trilinear lookup -----------
BAKED_LD = 24                     # floats per lattice point: the 22 channels padded to whole 16-byte pieces (include/fenerf.h)
BAKED_OUTSIDE_SIGMA = -1e30       # density of a sample outside the lattice: finite, and weight exactly 0 under relu and softplus alike


def baked_cube_length(fov, ray_start, ray_end, radius=1.0, num_steps=None):
    """Side of the smallest origin-centred cube that holds every sample of every ray for ANY yaw and pitch of a camera on the sphere of
    `radius` looking at the origin: two times the largest distance from the origin of a sample on a corner ray (the pixel grid spans
    [-1, 1]^2 at depth 1 / tan(fov / 2), so tan(theta_c) = sqrt(2) tan(fov / 2)) at depth ray_start or ray_end.  Pure host arithmetic.
    num_steps: the stratified jitter moves a sample by up to half a bin, (ray_end - ray_start) / (num_steps - 1) / 2, beyond either end
    (perturb_points); given the coarse sample count the cube holds the jittered samples too (the resampled depths lie between coarse
    samples).  Without it the cube holds the unjittered depths; a sample the jitter pushes past it renders as empty space."""
    import math
    margin = 0.0 if num_steps is None or num_steps < 2 else (ray_end - ray_start) / (num_steps - 1) / 2
    cos_c = 1.0 / math.sqrt(1.0 + 2.0 * math.tan(math.radians(fov) / 2) ** 2)
    far = max(math.sqrt(radius * radius + z * z - 2.0 * radius * z * cos_c) for z in (ray_start - margin, ray_end + margin))
    return 2.0 * far


class BakedField:
    """One identity's radiance field on a lattice (bake_field): vol [n0,n1,n2,ld] on the device, the first C floats of a lattice point =
    the SIREN's row [labels | rgb | sigma] under a locked view direction; lattice point i_k of axis k lies at origin[k] + i_k * spacing[k]
    (coordinate column k).  film = the (freq_geo, phase_geo, freq_app, phase_app) it was baked from.  An approximation: trilinear
    interpolation at the lattice's resolution stands in for the network."""

    def __init__(self, vol, origin, spacing, C, film, outside_last=BAKED_OUTSIDE_SIGMA):
        self.vol, self.origin, self.spacing = vol, tuple(float(x) for x in origin), tuple(float(x) for x in spacing)
        self.C, self.ld = int(C), int(vol.shape[-1])
        self.film = film
        self.outside_last = float(outside_last)

    def sample(self, points):
        """points [..., 3] on the device -> rows [..., C] (native.volume_sample)"""
        if torch.is_grad_enabled() and points.requires_grad:
            raise RuntimeError("BakedField.sample: the baked route is no-grad only")
        return native.volume_sample(self.vol, self.origin, self.spacing, points, self.outside_last, self.C)

    def _field_render(self, origins, dirs, z_coarse, u, noise_coarse, noise_final, fg, pg, fa, pa, opts, hierarchical=True, lock_view=False,
                      want_weights=False, want_wsum=False):
        """NativeModel.render's signature: the FiLM parameters and the view direction are baked in"""
        return native.volume_render(self.vol, self.origin, self.spacing, origins, dirs, z_coarse, u, noise_coarse, noise_final, opts,
                                    self.outside_last, self.C, hierarchical=hierarchical, want_weights=want_weights, want_wsum=want_wsum)

    def render(self, generator, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean, v_mean, hierarchical_sample=True,
               sample_dist=None, **kwargs):
        """staged_forward_with_frequencies(lock_view_dependence=True) of the baked identity with the two SIREN passes replaced by lattice
        lookups: the generator's own _render (the same rays, draws in the same order, composite options, fill modes) and image epilogue.
        -> (pixels [B,C',S,S], depth [B,S,S], third) on the CPU, as staged_forward_with_frequencies returns them.  No-grad only."""
        tensors = [t for t in (*self.film, h_mean, v_mean) if isinstance(t, torch.Tensor)]
        if any(t.requires_grad for t in tensors):
            raise RuntimeError("BakedField.render: the baked route is no-grad only (a FiLM tensor or a pose requires grad)")
        for k in ("psi", "lock_view_dependence", "max_batch_size", "depth_map", "near_clip", "far_clip"):      # staged_forward's own arguments
            kwargs.pop(k, None)
        B = self.film[0].shape[0]
        with torch.no_grad():
            pixels, depth, third, _, _ = generator._render(self.film, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean,
                                                           v_mean, hierarchical_sample, sample_dist, True, kwargs, use_fill=True, third="auto",
                                                           field_render=self._field_render)
            depth_map = native.to_host(depth.reshape(B, img_size, img_size).contiguous())
            third = native.to_host(third.reshape((B, img_size, img_size, -1)).permute(0, 3, 1, 2).contiguous() * 2 - 1)
            pixels = native.to_host(generator._finish_scaled(pixels, B, img_size))
        return pixels, depth_map, third

    def render_geometry(self, generator, *, light=(0, 0, 1), ambient=0.25, background=1.0, alpha_min=0.5, space="camera", details=False,
                        **render_kwargs):
        """render() plus the geometry of the view (callers.render_geometry, baked route): normals from the central difference of the
        lattice's density (native.volume_sample_grad on channel C - 1) at the rays' surface points.  -> the dict of render_geometry."""
        return _render_geometry(generator, self.film, self, True, render_kwargs, light, ambient, background, alpha_min, space, details)


def _bake_film(who, generator, z_geo, z_app, film, psi):
    """the FiLM parameters a lattice is baked from, exactly as extract_mesh: the truncated z route or film= -> (fg, pg, fa, pa), device"""
    siren = generator.siren
    if film is None:
        z_app = z_geo if z_app is None else z_app
        device = z_geo.device
        avg_fg, avg_pg, avg_fa, avg_pa = generator.generate_avg_frequencies()
        raw_fg, raw_pg = siren.geo_mapping_network(z_geo)
        raw_fa, raw_pa = siren.app_mapping_network(z_app)
        fg, pg = avg_fg + psi * (raw_fg - avg_fg), avg_pg + psi * (raw_pg - avg_pg)
        fa, pa = avg_fa + psi * (raw_fa - avg_fa), avg_pa + psi * (raw_pa - avg_pa)
    else:
        device = generator.device
        fg, pg = film["truncated_frequencies_geo"], film["truncated_phase_shifts_geo"]
        fa, pa = film["truncated_frequencies_app"], film["truncated_phase_shifts_app"]
    if any(t.requires_grad for t in (fg, pg, fa, pa)):
        raise RuntimeError(f"{who}: the baked route is no-grad only (a FiLM tensor requires grad)")
    if fg.shape[0] != 1:
        raise ValueError(f"{who}: one identity per lattice (FiLM batch of 1)")
    return (fg, pg, fa, pa), torch.device(device)


def _bake_slabs(n, origin, spacing, device, max_points):
    """the points of an n^3 lattice, origin + i * spacing per coordinate column (one fp32 multiply, one fp32 add), in slabs of at most
    max_points points along axis 0 padded to whole 32-point tiles -> (a0, a1, points [P + pad, 3], P) per slab"""
    idx = torch.arange(n, dtype=torch.float32, device=device)
    sp = torch.tensor(spacing, dtype=torch.float32, device=device)
    axis = [idx * sp + torch.tensor(origin[k], dtype=torch.float32, device=device) for k in range(3)]      # origin + i * spacing
    slab = max(1, min(n, int(max_points) // (n * n)))
    for a0 in range(0, n, slab):
        a1 = min(n, a0 + slab)
        pts = torch.stack(torch.meshgrid(axis[0][a0:a1], axis[1], axis[2], indexing="ij"), dim=-1).reshape(-1, 3)
        P = pts.shape[0]
        pad = (-P) % 32
        if pad:
            pts = torch.cat([pts, pts[-1:].expand(pad, -1)])
        yield a0, a1, pts, P


def bake_field(generator, z_geo, z_app=None, *, film=None, resolution=256, center=(0, 0, 0), cube_length, psi=0.5, max_points=1 << 24):
    """Evaluates one identity's field ONCE on a resolution^3 lattice of the cube of side cube_length around `center` (baked_cube_length
    gives the side that holds a camera's samples) and keeps all C channels -> BakedField.  FiLM parameters exactly as extract_mesh: the
    truncated z route (generate_avg_frequencies, psi), or film= (the meta dict of sample_generator_wth_frequencies_phase_shifts; z_geo /
    z_app / psi are then ignored).  View direction locked to (0, 0, -1).  Lattice points are origin + i * spacing per coordinate column
    (one fp32 multiply, one fp32 add): the statement the sampler inverts.  Evaluated in slabs of at most max_points points along axis 0,
    padded to whole 32-point tiles.  Memory: resolution^3 x 96 bytes."""
    n = int(resolution)
    if n < 2:
        raise ValueError("bake_field: resolution must be at least 2")
    siren = generator.siren
    with torch.no_grad():
        (fg, pg, fa, pa), device = _bake_film("bake_field", generator, z_geo, z_app, film, psi)
        spacing = float(cube_length) / (n - 1)
        origin = tuple(float(c) - float(cube_length) / 2 for c in center)
        nat = siren.native(device)
        C_out = int(siren.output_dim)
        ld = max(BAKED_LD, (C_out + 3) // 4 * 4)
        vol = torch.zeros((n, n, n, ld), dtype=torch.float32, device=device)
        for a0, a1, pts, P in _bake_slabs(n, origin, spacing, device, max_points):
            rows = nat.siren_forward(pts[None].contiguous(), None, fg, pg, fa, pa)[0, :P]          # None = locked view dir
            vol[a0:a1, :, :, :C_out] = rows.reshape(a1 - a0, n, n, C_out)
            del rows, pts
    return BakedField(vol, origin, (spacing,) * 3, C_out, (fg, pg, fa, pa))


def _multiview_film(generator, z_geo, z_app, avg, kw):
    """staged_forward's truncated FiLM parameters (psi of the kwargs bag; avg = what generate_avg_frequencies returned for this view's
    generator state) as the meta dict bake_field / bake_density take"""
    avg_fg, avg_pg, avg_fa, avg_pa = avg
    with torch.no_grad():
        raw_fg, raw_pg = generator.siren.geo_mapping_network(z_geo)
        raw_fa, raw_pa = generator.siren.app_mapping_network(z_app)
        psi = kw.get("psi", 1)
        return dict(truncated_frequencies_geo=avg_fg + psi * (raw_fg - avg_fg), truncated_phase_shifts_geo=avg_pg + psi * (raw_pg - avg_pg),
                    truncated_frequencies_app=avg_fa + psi * (raw_fa - avg_fa), truncated_phase_shifts_app=avg_pa + psi * (raw_pa - avg_pa))


def _baked_multiview_field(generator, z_geo, z_app, avg, kw, resolution):
    """the lattice render_multiview's views read: staged_forward's truncated FiLM parameters, in the cube that holds the camera's samples"""
    film = _multiview_film(generator, z_geo, z_app, avg, kw)
    cube = baked_cube_length(kw["fov"], kw["ray_start"], kw["ray_end"], num_steps=kw["num_steps"])
    return bake_field(generator, None, film=film, resolution=resolution, cube_length=cube)


def _baked_inversion_field(generator, film, render_options, resolution):
    """the lattice the inversion renders read: film = film_from_inversion's (freq_geo, freq_app, phase_geo, phase_app)"""
    cube = baked_cube_length(render_options["fov"], render_options["ray_start"], render_options["ray_end"], num_steps=render_options["num_steps"])
    return bake_field(generator, None, film=_film_meta(film), resolution=resolution, cube_length=cube)


# ---- proposal lattice: bake an identity's DENSITY once, place every view's samples from it, evaluate the network there --
class DensityField:
    """One identity's density on a lattice (bake_density): vol [n0,n1,n2] on the device, lattice point i_k of axis k at origin[k] + i_k *
    spacing[k].  sigma depends on position alone, so the lattice serves every view, view-dependent colour included.  film = the (freq_geo,
    phase_geo, freq_app, phase_app) it was baked from: render() evaluates the network with them at the depths the lattice proposes."""

    def __init__(self, vol, origin, spacing, film, outside_last=BAKED_OUTSIDE_SIGMA):
        self.vol, self.origin, self.spacing = vol, tuple(float(x) for x in origin), tuple(float(x) for x in spacing)
        self.film = film
        self.outside_last = float(outside_last)

    def sample(self, points):
        """points [..., 3] on the device -> sigma [...] (native.volume_sample on the one-channel lattice)"""
        if torch.is_grad_enabled() and points.requires_grad:
            raise RuntimeError("DensityField.sample: the proposal route is no-grad only")
        return native.volume_sample(self.vol.unsqueeze(-1), self.origin, self.spacing, points, self.outside_last, 1)[..., 0]

    def _field_render(self, nat):
        def field(origins, dirs, z_coarse, u, noise_coarse, noise_final, fg, pg, fa, pa, opts, hierarchical=True, lock_view=False,
                  want_weights=False, want_wsum=False):
            """NativeModel.render's signature, fed the exact route's draws as they come: u as is, the first N columns of noise_final
            (noise is indexed by sorted position; N samples are composited)"""
            N = z_coarse.shape[-1]
            nf = noise_final[..., :N].contiguous() if noise_final is not None else None
            return nat.render_proposal(self.vol, self.origin, self.spacing, origins, dirs, z_coarse, u, noise_coarse, nf, fg, pg, fa, pa, opts,
                                       outside_last=self.outside_last, lock_view=lock_view, want_weights=want_weights, want_wsum=want_wsum)
        return field

    def render(self, generator, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean, v_mean, hierarchical_sample=True,
               sample_dist=None, lock_view_dependence=False, **kwargs):
        """staged_forward_with_frequencies of the baked identity with the coarse SIREN pass replaced by a lookup into the density lattice:
        the generator's own _render (the same rays, draws in the same order, composite options, fill modes) and image epilogue; the
        network is evaluated once per ray sample, at the N depths resampled from the lattice's weights, with the caller's view direction
        (lock_view_dependence as given).  -> (pixels [B,C',S,S], depth [B,S,S], third) on the CPU, as staged_forward_with_frequencies
        returns them (weights: [B,R,N]).  No-grad only."""
        if not hierarchical_sample:
            raise ValueError("DensityField.render: hierarchical_sample=False has no fine samples to propose; render it with the exact route")
        tensors = [t for t in (*self.film, h_mean, v_mean) if isinstance(t, torch.Tensor)]
        if any(t.requires_grad for t in tensors):
            raise RuntimeError("DensityField.render: the proposal route is no-grad only (a FiLM tensor or a pose requires grad)")
        for k in ("psi", "max_batch_size", "depth_map", "near_clip", "far_clip"):      # staged_forward's own arguments
            kwargs.pop(k, None)
        B = self.film[0].shape[0]
        with torch.no_grad():
            field = self._field_render(generator.siren.native(generator.device))
            pixels, depth, third, _, _ = generator._render(self.film, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean,
                                                           v_mean, True, sample_dist, bool(lock_view_dependence), kwargs, use_fill=True,
                                                           third="auto", field_render=field)
            depth_map = native.to_host(depth.reshape(B, img_size, img_size).contiguous())
            third = native.to_host(third.reshape((B, img_size, img_size, -1)).permute(0, 3, 1, 2).contiguous() * 2 - 1)
            pixels = native.to_host(generator._finish_scaled(pixels, B, img_size))
        return pixels, depth_map, third


def bake_density(generator, z_geo, z_app=None, *, film=None, resolution=256, center=(0, 0, 0), cube_length, psi=0.5, max_points=1 << 24):
    """Evaluates one identity's DENSITY once on a resolution^3 lattice of the cube of side cube_length around `center` -> DensityField.
    FiLM parameters, cube, lattice points and slabs exactly as bake_field; sigma from _lattice_sigma (the density route where the model
    serves it, else the full forward: the same bits).  Memory: resolution^3 x 4 bytes."""
    n = int(resolution)
    if n < 2:
        raise ValueError("bake_density: resolution must be at least 2")
    with torch.no_grad():
        (fg, pg, fa, pa), device = _bake_film("bake_density", generator, z_geo, z_app, film, psi)
        spacing = float(cube_length) / (n - 1)
        origin = tuple(float(c) - float(cube_length) / 2 for c in center)
        nat = generator.siren.native(device)
        vol = torch.empty((n, n, n), dtype=torch.float32, device=device)
        for a0, a1, pts, P in _bake_slabs(n, origin, spacing, device, max_points):
            sigma, _ = _lattice_sigma(nat, pts[None].contiguous(), fg, pg, fa, pa)
            vol[a0:a1] = sigma[0, :P].reshape(a1 - a0, n, n)
            del sigma, pts
    return DensityField(vol, origin, (spacing,) * 3, (fg, pg, fa, pa))


def _film_meta(film):
    """film_from_inversion's (freq_geo, freq_app, phase_geo, phase_app) as the meta dict bake_field / bake_density take"""
    return dict(truncated_frequencies_geo=film[0], truncated_frequencies_app=film[1], truncated_phase_shifts_geo=film[2], truncated_phase_shifts_app=film[3])


def _proposal_multiview_field(generator, z_geo, z_app, avg, kw, resolution):
    """_baked_multiview_field's density counterpart: the same FiLM parameters, the same cube"""
    film = _multiview_film(generator, z_geo, z_app, avg, kw)
    cube = baked_cube_length(kw["fov"], kw["ray_start"], kw["ray_end"], num_steps=kw["num_steps"])
    return bake_density(generator, None, film=film, resolution=resolution, cube_length=cube)


def _proposal_inversion_field(generator, film, render_options, resolution):
    """_baked_inversion_field's density counterpart"""
    cube = baked_cube_length(render_options["fov"], render_options["ray_start"], render_options["ray_end"], num_steps=render_options["num_steps"])
    return bake_density(generator, None, film=_film_meta(film), resolution=resolution, cube_length=cube)


def _refuse_proposal_with(who, proposal, **others):
    """proposal= places the samples of the exact colour render; it goes with none of the routes named in `others`"""
    if proposal is None:
        return
    taken = [k for k, v in others.items() if v is not None and v is not False]
    if taken:
        raise ValueError(f"{who}: proposal renders the network's own pixels at depths placed from a baked density lattice; it does not "
                         f"combine with {' / '.join(taken)}")
    if int(proposal) < 2:
        raise ValueError(f"{who}: proposal is a lattice resolution of at least 2")


# ---- geometry views: surface normals and a shaded "shape" image for the pixels of a render --------------------------
_RENDER_POSITIONALS = ("img_size", "fov", "ray_start", "ray_end", "num_steps", "h_stddev", "v_stddev", "h_mean", "v_mean")


def _unit_light(light):
    """the light direction normalised on the host (float64), as the three floats the kernel uses as given"""
    l = np.asarray(light, dtype=np.float64).reshape(3)
    norm = float(np.linalg.norm(l))
    if not (np.isfinite(norm) and norm > 0):
        raise ValueError(f"render_geometry: light must be a finite non-zero direction, not {light!r}")
    return tuple(float(x) for x in (l / norm).astype(np.float32))


def _render_geometry(generator, film, field, lock_view, render_kwargs, light, ambient, background, alpha_min, space, details):
    """film = (freq_geo, phase_geo, freq_app, phase_app); field = a BakedField (lattice lookups and lattice normals) or None (the SIREN)"""
    from .generators.volumetric_rendering import create_cam2world_matrix, normalize_vecs
    if space not in ("camera", "world"):
        raise ValueError(f'render_geometry: space is "camera" or "world", not {space!r}')
    light = _unit_light(light)
    kw = dict(render_kwargs)
    missing = [k for k in _RENDER_POSITIONALS if k not in kw]
    if missing:
        raise TypeError(f"render_geometry: missing render arguments {missing}")
    img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean, v_mean = (kw.pop(k) for k in _RENDER_POSITIONALS)
    hierarchical = kw.pop("hierarchical_sample", field is not None)          # the defaults of staged_forward* / BakedField.render
    sample_dist = kw.pop("sample_dist", None)
    for k in ("psi", "lock_view_dependence", "max_batch_size", "depth_map", "near_clip", "far_clip"):      # staged_forward's own arguments
        kw.pop(k, None)
    if any(isinstance(t, torch.Tensor) and t.requires_grad for t in (*film, h_mean, v_mean)):
        raise RuntimeError("render_geometry: a geometry view is no-grad only (a FiLM tensor or a pose requires grad)")
    B, R = film[0].shape[0], img_size * img_size
    rays = {}
    with torch.no_grad():
        pixels, depth, _, _, _ = generator._render(film, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean, v_mean,
                                                   hierarchical, sample_dist, lock_view, kw, use_fill=True, third="wsum",
                                                   field_render=None if field is None else field._field_render, rays_out=rays)
        wsum = rays["wsum"]
        alpha = None if kw.get("last_back", False) else wsum          # last_back: the weights already sum to one
        points = native.surface_points(rays["origins"], rays["dirs"], depth, alpha, alpha_min)
    if field is None:
        chunk = max(32, MESH_NORMAL_CHUNK // max(B, 1) // 32 * 32)
        try:
            grads = _sigma_input_grads(generator.siren, points, *film, chunk)
        except native._lib.FenerfError as e:
            if "bf16" in str(e):
                raise RuntimeError("render_geometry: this model's precision tier writes the bf16 gradient dump at this size (wgrad_bf16_min_points), "
                                   "which the input-gradient pass cannot read; render the geometry view with an fp32-dump model or with baked=") from e
            raise
    else:
        grads = native.volume_sample_grad(field.vol, field.origin, field.spacing, points, field.C - 1)
    with torch.no_grad():
        cam2world = None
        if space == "camera":
            cam = rays["origins"][:, 0]
            cam2world = create_cam2world_matrix(normalize_vecs(-cam), cam)[:, :3, :3].contiguous()
        normals, shaded = native.shade_normals(grads, R, alpha, cam2world, light, ambient, background, alpha_min)
        S = img_size
        out = dict(pixels=native.to_host(generator._finish_scaled(pixels, B, S)), depth=native.to_host(depth.reshape(B, S, S).contiguous()),
                   alpha=native.to_host(wsum.reshape(B, S, S).contiguous()),
                   normal=native.to_host(normals.reshape(B, S, S, 3).permute(0, 3, 1, 2).contiguous()),
                   shaded=native.to_host(shaded.reshape(B, 1, S, S).contiguous()))
        if details:
            out.update(origins=native.to_host(rays["origins"].contiguous()), dirs=native.to_host(rays["dirs"].contiguous()), points=native.to_host(points),
                       grad=native.to_host(grads.contiguous()), cam2world=None if cam2world is None else native.to_host(cam2world))
    return out


def render_geometry(generator, z_geo=None, z_app=None, *, film=None, baked=None, light=(0, 0, 1), ambient=0.25, background=1.0, alpha_min=0.5,
                    space="camera", details=False, **render_kwargs):
    """A render and the geometry of its pixels: a normal map and a Lambert-shaded "shape" image.
    The render is staged_forward's (z_geo / z_app, truncated with psi -- staged_forward's default 1) or, with film= (the meta dict of
    sample_generator_wth_frequencies_phase_shifts), staged_forward_with_frequencies': the same rays, draws and launches; render_kwargs are
    that call's arguments.  Per ray the surface point is origin + dir * (depth / alpha) where the weight sum alpha >= alpha_min (depth
    itself otherwise, and under last_back), the normal is -grad(sigma) / |grad(sigma)| there, and the shaded value is
    ambient + (1 - ambient) * max(n . light, 0), alpha-blended onto `background`; rays with alpha < alpha_min get a zero normal and
    `background` (native.surface_points / shade_normals, include/fenerf.h "geometry views").
    baked=None: grad(sigma) is the SIREN's own input gradient at the R surface points (extract_mesh's normal route: forward-save, chain,
    input-gradient pass).  baked= a BakedField or a lattice resolution: the render is BakedField.render's (view direction locked) and
    grad(sigma) the central difference of the lattice (native.volume_sample_grad): an approximation, and no SIREN launch per view.
    space="camera": normals in the view's camera frame (x right, y up, z towards the camera); "world": as the field has them.
    `light` is normalised on the host.  No-grad only.
    -> dict on the CPU: pixels [B,C',S,S], depth [B,S,S] (exactly the staged call's), alpha [B,S,S] (the weight sum), normal [B,3,S,S],
    shaded [B,1,S,S]; details=True adds origins, dirs [B,R,3], points, grad [B,Pp,3] (Pp = R rounded up to 32) and cam2world [B,3,3]."""
    kw = dict(render_kwargs)
    siren = generator.siren
    if isinstance(baked, BakedField):
        return baked.render_geometry(generator, light=light, ambient=ambient, background=background, alpha_min=alpha_min, space=space, details=details, **kw)
    with torch.no_grad():
        if film is None:
            if z_geo is None:
                raise TypeError("render_geometry: give z_geo (and z_app), film= or a BakedField")
            z_app = z_geo if z_app is None else z_app
            psi = kw.get("psi", 1)
            avg_fg, avg_pg, avg_fa, avg_pa = generator.generate_avg_frequencies()
            raw_fg, raw_pg = siren.geo_mapping_network(z_geo)
            raw_fa, raw_pa = siren.app_mapping_network(z_app)
            fg, pg = avg_fg + psi * (raw_fg - avg_fg), avg_pg + psi * (raw_pg - avg_pg)
            fa, pa = avg_fa + psi * (raw_fa - avg_fa), avg_pa + psi * (raw_pa - avg_pa)
        else:
            fg, pg = film["truncated_frequencies_geo"], film["truncated_phase_shifts_geo"]
            fa, pa = film["truncated_frequencies_app"], film["truncated_phase_shifts_app"]
    if baked is not None:
        meta = dict(truncated_frequencies_geo=fg, truncated_phase_shifts_geo=pg, truncated_frequencies_app=fa, truncated_phase_shifts_app=pa)
        cube = baked_cube_length(kw["fov"], kw["ray_start"], kw["ray_end"], num_steps=kw["num_steps"])
        field = bake_field(generator, None, film=meta, resolution=int(baked), cube_length=cube)
        return field.render_geometry(generator, light=light, ambient=ambient, background=background, alpha_min=alpha_min, space=space, details=details, **kw)
    return _render_geometry(generator, (fg, pg, fa, pa), None, bool(kw.get("lock_view_dependence", False)), kw, light, ambient, background, alpha_min,
                            space, details)


# ---- the inversion script's host pieces (inverse_render_double_semantic.py) ------------------------------------------------------------
COLOR_MAP_COMPLETE_KEYS = 19      # labels 0 (background) .. 18 of the script's COLOR_MAP_COMPLETE (:50-69); COLOR_MAP has 1 .. 18


def mask2labels(mask_np, n_labels=18):
    """One-hot [n_labels, H, W] float64 of a label image (:82-92): 19 labels -> channel i is label i; 18 -> channel i is label i + 1
    (background dropped)."""
    labels = np.zeros((n_labels, mask_np.shape[0], mask_np.shape[1]))
    for i in range(n_labels):
        labels[i][mask_np == (i if n_labels == 19 else i + 1)] = 1.0
    return labels


def mIOU(source, target):
    """(:122-126) mean over classes of |s * t| / (|s + t > 0| + 1e-6), per image"""
    return torch.mean(torch.div(torch.sum(source * target, dim=[2, 3]).float(), torch.sum((source + target) > 0, dim=[2, 3]).float() + 1e-6), dim=1)


def _pil_resize_shorter(img, size, resample):
    """torchvision.transforms.Resize(int) on a PIL image: the shorter side becomes `size`, the other int(size * long / short)"""
    w, h = img.size
    if (w <= h and w == size) or (h <= w and h == size):
        return img
    if w < h:
        return img.resize((size, int(size * h / w)), resample)
    return img.resize((int(size * w / h), size), resample)


def _pil_center_crop(img, size):
    """torchvision.transforms.CenterCrop(size) for an image at least that large: left/top = round((dim - size) / 2)"""
    w, h = img.size
    left, top = int(round((w - size) / 2.0)), int(round((h - size) / 2.0))
    return img.crop((left, top, left + size, top + size))


def _pil_to_tensor(img):
    """transforms.ToTensor(): [C, H, W] float in [0, 1] ('L' -> one channel)"""
    a = np.asarray(img, dtype=np.uint8)
    a = a[:, :, None] if a.ndim == 2 else a
    return torch.from_numpy(np.array(a.transpose(2, 0, 1))).float().div(255)


def inversion_targets(gt_image, gt_seg, image_size=256, no_center_crop=False, background_mask=False, white_background_mask=False):
    """The targets of one inversion from two PIL images -- an RGB photo and its 'L' label map (values 0 .. 18) -- as
    inverse_render_double_semantic.py:178-222, :290-327 builds them with torchvision transforms (restated on PIL directly: Resize(320,
    bilinear) -> CenterCrop(256) -> Resize((S, S), NEAREST) -> ToTensor [-> Normalize(0.5, 0.5)]; `no_center_crop`: the last resize only):
    -> gt_image [1,3,S,S] in [-1,1], gt_seg_18 [1,18,S,S] in {-1,1}, gt_seg_19 [1,19,256,256] in {0,1} (the mIoU target, always 256^2).
    background_mask / white_background_mask paint the photo 0 / 1 where the label map is 0 (:295-310)."""
    from PIL import Image
    gt_image, gt_seg = gt_image.convert("RGB"), gt_seg.convert("L")
    if background_mask or white_background_mask:
        i = _pil_to_tensor(gt_image)
        lab = _pil_to_tensor(gt_seg.resize(gt_image.size, resample=Image.NEAREST)) * 255.0
        i[lab.expand_as(i) == 0] = 0.0 if background_mask else 1.0
        gt_image = Image.fromarray(i.mul(255).byte().permute(1, 2, 0).numpy())     # transforms.ToPILImage() of a float tensor: mul(255).byte()

    def pipeline(img, size):
        if not no_center_crop:
            img = _pil_center_crop(_pil_resize_shorter(img, 320, Image.BILINEAR), 256)
        return _pil_to_tensor(img.resize((size, size), Image.NEAREST))

    image = (pipeline(gt_image, image_size) - 0.5) / 0.5
    seg18 = (torch.tensor(mask2labels((pipeline(gt_seg, image_size) * 255.0)[0].numpy(), 18), dtype=torch.float) - 0.5) / 0.5
    seg19 = torch.tensor(mask2labels((pipeline(gt_seg, 256) * 255.0)[0].numpy(), 19), dtype=torch.float)
    return image[None], seg18[None], seg19[None]


def inversion_options(image_size=256, fov=12, device=None):
    """The kwargs bag of the optimisation renders (:225-247): 24 coarse samples only, frontal camera, eval fill mode"""
    import math
    hv = torch.tensor(math.pi / 2)
    hv = hv.to(device) if device is not None else hv
    return {'img_size': image_size, 'fov': fov, 'ray_start': 0.88, 'ray_end': 1.12, 'num_steps': 24, 'h_stddev': 0, 'v_stddev': 0,
            'h_mean': hv, 'v_mean': hv.clone(), 'hierarchical_sample': False, 'sample_dist': None, 'clamp_mode': 'relu', 'nerf_noise': 0,
            'fade_steps': 10000, 'z_app_lambda': 0, 'z_geo_lambda': 0, 'pos_lambda': 0, 'tok_interval': 2000, 'tok_v': 0.6, 'betas': (0, 0.9),
            'fill_mode': 'eval_seg_padding_background'}


def inversion_render_options(fov=12, fill_color='black', img_size=256, num_steps=48):
    """The kwargs bag of the preview / reconstruction renders (:249-265): 256^2, 48 + 48 samples"""
    import math
    return {'img_size': img_size, 'fov': fov, 'ray_start': 0.88, 'ray_end': 1.12, 'num_steps': num_steps, 'h_stddev': 0, 'v_stddev': 0,
            'v_mean': math.pi / 2, 'hierarchical_sample': True, 'sample_dist': None, 'clamp_mode': 'relu', 'nerf_noise': 0, 'last_back': False,
            'fill_mode': 'eval_seg_padding_background', 'fill_color': fill_color}


def inversion_trajectory(name, num_frames, fov):
    """[(t, pitch, yaw, fov)] of the inversion script's set_trajectory (:504-570): the video script's trajectories plus 'inverse_sphere'
    and 'rotation_linear'; its 'zoom' runs t over linspace(-1, 1) (50 frames whatever num_frames says) with fov + 5 + 5 sin(2 pi t)."""
    pi = np.pi
    if name in ("front", "orbit", "non_rotation", "sphere", "rotation_horizontal"):
        return camera_trajectory(name, num_frames, fov)
    if name == "inverse_sphere":
        return [(t, 0.2 * (1 - np.cos(t * 2 * pi)) + pi / 2, 0.4 * np.sin(t * 2 * pi) + pi / 2, fov) for t in np.linspace(0, 1, num_frames)]
    if name == "zoom":
        return [(t, pi / 2, pi / 2, fov + 5 + np.sin(t * 2 * pi) * 5) for t in np.linspace(-1, 1)]
    if name == "rotation_linear":
        return [(t, pi / 2, pi / 2 + t, fov) for t in np.linspace(-0.4, 0.4, num_frames)]
    raise ValueError(f"unknown trajectory {name!r} (front | orbit | non_rotation | sphere | inverse_sphere | rotation_horizontal | zoom | rotation_linear)")


def _inversion_pose(pose):
    """(yaw, pitch) as floats, or None: the reference's frontal pi / 2"""
    return None if pose is None else (float(pose[0]), float(pose[1]))


def render_inversion_views(generator, meta, render_options, angles=(0.0,), max_batch_size=2400000, lock_view_dependence=False, pose=None, baked=None,
                           proposal=None):
    """staged_forward_with_frequencies of an inversion state at yaws pi/2 + angle (:419-431, :441-446) -> [(angle, frame [1,22,S,S])].
    pose: (yaw, pitch) to centre the angles on instead -- what inverse_render(optimize_pose=True) recovered.
    baked: a lattice resolution -- bake the inverted identity once (view direction locked) and render every view from the lattice
    (BakedField.render: an approximation).  None = the exact renders.
    proposal: a lattice resolution -- bake the inverted identity's density once and place every view's samples from it (DensityField.render,
    INTEGRATION.md L; lock_view_dependence is honoured).  Not with baked."""
    import math
    _refuse_proposal_with("render_inversion_views", proposal, baked=baked)
    film = film_from_inversion(meta)
    pose = _inversion_pose(pose)
    if pose is not None:
        render_options = dict(render_options, v_mean=pose[1])
    centre = math.pi / 2 if pose is None else pose[0]
    out = []
    with torch.no_grad():
        field = None if baked is None else _baked_inversion_field(generator, film, render_options, baked)
        if proposal is not None:
            field = _proposal_inversion_field(generator, film, render_options, proposal)
        for angle in angles:
            if field is not None:
                img, _, _ = field.render(generator, h_mean=centre + angle, lock_view_dependence=lock_view_dependence, **render_options)
            else:
                img, _, _ = generator.staged_forward_with_frequencies(*film, h_mean=centre + angle, max_batch_size=max_batch_size,
                                                                      lock_view_dependence=lock_view_dependence, **render_options)
            out.append((angle, img))
    return out


def render_inversion_recon(generator, meta, render_options, trajectory, max_batch_size=2400000, lock_view_dependence=False, pose=None, baked=None,
                           proposal=None):
    """The frames of run_render_recon_video (:462-501): per trajectory entry one staged render of the inverted identity at (pitch, yaw) --
    the trajectory's fov is NOT applied (the reference sets only h_mean / v_mean) -- as uint8 [S, 3 S, 3] RGB panels
    [image | label colours | 0.5 / 0.5 blend] (the reference hands them to cv2 as BGR).
    pose: (yaw, pitch) the trajectory -- written around the frontal (pi / 2, pi / 2) -- is moved to: what inverse_render(optimize_pose=True)
    recovered.  baked: a lattice resolution -- bake once, render every frame from the lattice (as render_inversion_views).
    proposal: a lattice resolution -- bake the density once, place every frame's samples from it (as render_inversion_views); not with baked."""
    import math
    from . import imageio_lite
    _refuse_proposal_with("render_inversion_recon", proposal, baked=baked)
    film = film_from_inversion(meta)
    pose = _inversion_pose(pose)
    d_yaw, d_pitch = (0.0, 0.0) if pose is None else (pose[0] - math.pi / 2, pose[1] - math.pi / 2)
    kw = dict(render_options)
    frames = []
    to_u8 = lambda t: imageio_lite.to_uint8_hwc(imageio_lite.make_grid(t, normalize=True))     # tensor_to_PIL (:114-119)
    with torch.no_grad():
        field = None if baked is None else _baked_inversion_field(generator, film, kw, baked)
        if proposal is not None:
            field = _proposal_inversion_field(generator, film, kw, proposal)
        for _, pitch, yaw, _ in trajectory:
            kw.update(h_mean=float(yaw) + d_yaw, v_mean=float(pitch) + d_pitch)
            if field is not None:
                frame, _, _ = field.render(generator, lock_view_dependence=lock_view_dependence, **kw)
            else:
                frame, _, _ = generator.staged_forward_with_frequencies(*film, max_batch_size=max_batch_size, lock_view_dependence=lock_view_dependence, **kw)
            image, sem = to_u8(frame[:, -3:].cpu()), to_u8(mask2color(frame[:, :-3], generator.device))
            blend = image * 0.5 + sem * 0.5
            frames.append(np.concatenate([image, sem, blend], axis=1).astype("uint8"))
    return frames


def inverse_render(generator, gt_image, gt_seg, options, n_iterations=700, init_psi=0.0, lambda_seg=1.0, lambda_img=1.0,
                   lambda_percept=0.0, lambda_norm=0.0, percept=None, z_dim=256, lr=1e-2, on_step=None, latent_noise=0.03,
                   n_mean_latents=10000, record_offsets=False, optimize_pose=False, lr_pose=None, init_pose=None, gt_depth=None, depth_mask=None,
                   lambda_depth=0.0, pose_model="angles", optimize_focal=False):
    """GAN inversion in FiLM space (inverse_render_double_semantic.py:306-410): optimise additive offsets on the geometry /
    appearance frequencies and phase shifts with Adam (lr 1e-2, weight_decay 1e-4, StepLR(100, 0.75)) under annealed
    latent noise so that generator.forward_with_frequencies reproduces gt_image [1,3,S,S] and gt_seg [1,18,S,S] (both in
    [-1,1]).  Every iteration is a native differentiable render; when the generator's parameters do not require grad
    only the FiLM gradients are computed.  `percept` (e.g. an LPIPS module) is optional -- none is shipped.
    Every draw (the mean-latent blocks -- `n_mean_latents` = 10,000 in the script --, the random latents, the four noise tensors of an
    iteration) goes through generator.draws in the script's order: with the default source that is torch.randn / randn_like on the
    device, value for value the script's generator consumption; a test replays the draws the reference recorded.
    Returns a dict with the reference's checkpoint keys (w_*_frequencies, w_*_phase_shifts, w_*_offsets) + `losses`
    (+ `offset_history`: the four offset tensors after every iteration, on the host, if record_offsets) + `yaw` / `pitch`.
    optimize_pose: the camera's yaw / pitch (options['h_mean'] / ['v_mean'], or init_pose = (yaw, pitch)) are optimised with the offsets --
    what the reference leaves to an external pose estimate (its hand-over is commented out, :422-423, :440, :490-491): leaf parameters in
    an Adam group of their own (lr_pose, default lr; no weight decay -- an angle has no reason to shrink towards 0), through the rays'
    gradient of the differentiable render.  Off: every value and draw is what it was; `yaw` / `pitch` report the options' pose.
    gt_depth [1,S,S] (an RGB-D capture, a second view's geometry; depth_mask [1,S,S] or None = every pixel) with lambda_depth > 0 adds
    lambda_depth * mean(mask * |depth - gt_depth|) on the render's depth map, which then carries the graph
    (forward_with_frequencies(return_depth=True)); the result gains `depth_losses`, the unweighted term per iteration.  With the defaults
    the loop is what it was: no return_depth, the same launches.
    pose_model (with optimize_pose): "angles" -- the two angles above, the default -- or "se3": a free camera (fenerf_amd.camera) around
    the options' pose, Camera.from_angles(yaw, pitch, fov).perturbed(rotvec, shift, log_focal) with rotvec / shift [1,3] (and log_focal [1]
    with optimize_focal) starting at zero in the pose Adam group: roll, distance and translation (and focal length) move too.  Every
    iteration renders through generator.forward_camera_with_frequencies; the draws are the angle route's.  The result and on_step's dict
    then carry `cam2world` [1,3,4] / `intrinsics` [1,5] (detached), and `yaw` / `pitch` report the pose the camera started from."""
    if pose_model not in ("angles", "se3"):
        raise ValueError(f"inverse_render: pose_model {pose_model!r} (angles | se3)")
    if pose_model == "se3" and not optimize_pose:
        raise ValueError("inverse_render: pose_model='se3' is a model of the optimised pose; set optimize_pose=True")
    if optimize_focal and pose_model != "se3":
        raise ValueError("inverse_render: optimize_focal needs pose_model='se3' (the angle camera has one fixed fov)")
    se3 = optimize_pose and pose_model == "se3"
    device = generator.device
    siren = generator.siren
    draws = generator.draws

    def init(mapping):     # :307-327
        z = draws.randn((n_mean_latents, z_dim), device)
        rand_z = draws.randn((1, z_dim), device)
        with torch.no_grad():
            freq, phase = mapping(z)
            rand_f, rand_p = mapping(rand_z)
        w_f, w_p = freq.mean(0, keepdim=True), phase.mean(0, keepdim=True)
        w_f = w_f + init_psi * (rand_f - w_f)
        w_p = w_p + init_psi * (rand_p - w_p)
        return w_f, w_p, torch.zeros_like(w_f).requires_grad_(), torch.zeros_like(w_p).requires_grad_()

    w_gf, w_gp, o_gf, o_gp = init(siren.geo_mapping_network)
    w_af, w_ap, o_af, o_ap = init(siren.app_mapping_network)
    if lambda_img == 0:        # :371-376
        opt_params = [o_gf, o_gp]
    elif lambda_seg == 0:
        opt_params = [o_af, o_ap]
    else:
        opt_params = [o_gf, o_gp, o_af, o_ap]
    yaw, pitch = options.get("h_mean"), options.get("v_mean")
    base_camera = pose_params = None
    if se3:
        from .camera import Camera
        if init_pose is not None:
            yaw, pitch = init_pose
        S = options["img_size"]
        with torch.no_grad():
            base_camera = Camera.from_angles(yaw, pitch, options["fov"], (S, S), device=device)
        rotvec, shift = (torch.zeros((1, 3), device=device).requires_grad_() for _ in range(2))
        log_focal = torch.zeros((1,), device=device).requires_grad_() if optimize_focal else None
        pose_params = [rotvec, shift] + ([log_focal] if optimize_focal else [])
        camera_options = {k: v for k, v in options.items() if k not in _ANGLE_CAMERA_KEYS}
        opt_params = [dict(params=opt_params), dict(params=pose_params, lr=lr if lr_pose is None else lr_pose, weight_decay=0.0)]
    elif optimize_pose:
        leaf = lambda v: torch.as_tensor(v, dtype=torch.float32).detach().to(device).reshape(()).clone().requires_grad_()
        yaw, pitch = leaf(yaw if init_pose is None else init_pose[0]), leaf(pitch if init_pose is None else init_pose[1])
        options = dict(options, h_mean=yaw, v_mean=pitch)
        opt_params = [dict(params=opt_params), dict(params=[yaw, pitch], lr=lr if lr_pose is None else lr_pose, weight_decay=0.0)]
    pose_now = lambda: dict(yaw=yaw.detach().clone() if optimize_pose and not se3 else yaw,
                            pitch=pitch.detach().clone() if optimize_pose and not se3 else pitch)

    def camera_now():
        with torch.no_grad():
            c = base_camera.perturbed(rotvec, shift, log_focal)
        return dict(cam2world=c.cam2world.clone(), intrinsics=c.intrinsics.clone())
    optimizer = torch.optim.Adam(opt_params, lr=lr, weight_decay=1e-4)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, 100, gamma=0.75)
    mse = torch.nn.MSELoss(reduction="mean")
    losses, history, depth_losses = [], [], []
    use_depth = gt_depth is not None and lambda_depth != 0
    if use_depth:
        gt_depth = torch.as_tensor(gt_depth, dtype=torch.float32).to(device)
        depth_mask = None if depth_mask is None else torch.as_tensor(depth_mask).to(device=device, dtype=torch.float32)
    for i in range(n_iterations):
        k = (n_iterations - i) / n_iterations                     # annealed noise on the FiLM parameters (:381-384; 0.03 there)
        # draw order and arithmetic of the reference (:381-384): geo freq, geo phase, app freq, app phase; (0.03 * randn) * k
        n_gf, n_gp = latent_noise * draws.randn(tuple(w_gf.shape), device) * k, latent_noise * draws.randn(tuple(w_gp.shape), device) * k
        n_af, n_ap = latent_noise * draws.randn(tuple(w_af.shape), device) * k, latent_noise * draws.randn(tuple(w_ap.shape), device) * k
        if se3:
            out = generator.forward_camera_with_frequencies(w_gf + n_gf + o_gf, w_af + n_af + o_af, w_gp + n_gp + o_gp, w_ap + n_ap + o_ap,
                                                            base_camera.perturbed(rotvec, shift, log_focal), return_depth=use_depth,
                                                            **camera_options)
            frame, depth = out[0], (out[2] if use_depth else None)
        elif use_depth:
            frame, _, depth = generator.forward_with_frequencies(w_gf + n_gf + o_gf, w_af + n_af + o_af, w_gp + n_gp + o_gp, w_ap + n_ap + o_ap,
                                                                 return_depth=True, **options)
        else:
            frame, _ = generator.forward_with_frequencies(w_gf + n_gf + o_gf, w_af + n_af + o_af, w_gp + n_gp + o_gp, w_ap + n_ap + o_ap,
                                                          **options)
        loss = lambda_seg * mse(frame[:, :-3], gt_seg) + lambda_img * mse(frame[:, -3:], gt_image)
        if use_depth:
            err = (depth - gt_depth.reshape(depth.shape)).abs()
            depth_term = (err if depth_mask is None else err * depth_mask.reshape(depth.shape)).mean()
            loss = loss + lambda_depth * depth_term
            depth_losses.append(depth_term.detach())
        if lambda_percept and percept is not None:
            loss = loss + lambda_percept * percept(frame[:, -3:], gt_image).sum()
        if lambda_norm > 0:
            loss = loss + lambda_norm * sum((o ** 2).mean() for o in (o_gf, o_gp, o_af, o_ap))
        loss.backward()
        optimizer.step()
        optimizer.zero_grad()
        scheduler.step()
        # the loss stays on the device unless a callback wants it now: reading it every iteration makes the host wait for the step it has
        # just enqueued, and the next iteration's launches then start from an idle device
        losses.append(loss.detach() if on_step is None else float(loss.detach()))
        if record_offsets:
            history.append(tuple(o.detach().cpu().clone() for o in (o_gf, o_gp, o_af, o_ap)))
        if on_step is not None:      # (i, loss, the reference's checkpoint dict at this iteration: what its in-loop preview renders use, :419-452)
            on_step(i, losses[-1], dict(w_geo_frequencies=w_gf, w_geo_phase_shifts=w_gp, w_app_frequencies=w_af, w_app_phase_shifts=w_ap,
                                        w_geo_frequency_offsets=o_gf.detach(), w_geo_phase_shift_offsets=o_gp.detach(),
                                        w_app_frequency_offsets=o_af.detach(), w_app_phase_shift_offsets=o_ap.detach(), **pose_now(),
                                        **(camera_now() if se3 else {})))
    if losses and on_step is None:
        losses = torch.stack(losses).cpu().tolist()
    extra = dict(offset_history=history) if record_offsets else {}
    if use_depth:
        extra["depth_losses"] = torch.stack(depth_losses).cpu().tolist() if depth_losses else []
    if se3:
        extra.update(camera_now())
    return dict(**extra, w_geo_frequencies=w_gf, w_geo_phase_shifts=w_gp, w_app_frequencies=w_af, w_app_phase_shifts=w_ap,
                w_geo_frequency_offsets=o_gf.detach(), w_geo_phase_shift_offsets=o_gp.detach(),
                w_app_frequency_offsets=o_af.detach(), w_app_phase_shift_offsets=o_ap.detach(), losses=losses,
                **{k: (None if v is None else float(v)) for k, v in pose_now().items()})


def render_latent_interpolation(generator, z1_geo, z2_geo, z1_app, z2_app, options, n_frames=8, latent_type="both", psi=1.0,
                                trajectory=None):
    """Frames of a walk between two identities in FiLM space (render_video_interpolation_semantic.py:131-187, :314-380):
    truncate both ends towards the mean FiLM parameters, interpolate the geometry and / or appearance side linearly
    ('geo' | 'app' | 'both' | 'non'; 'app' sweeps t over [-1, 1] like the reference), render every frame with
    staged_forward_with_frequencies.  trajectory: optional list of (pitch, yaw) per frame overriding v_mean / h_mean.
    -> (frames [F, C, S, S], depth [F, S, S]) on the CPU."""
    avg_fg, avg_pg, avg_fa, avg_pa = generator.generate_avg_frequencies()
    trunc = lambda avg, raw: avg + psi * (raw - avg)
    with torch.no_grad():
        ends = []
        for zg, za in ((z1_geo, z1_app), (z2_geo, z2_app)):
            fg, pg = generator.siren.geo_mapping_network(zg)
            fa, pa = generator.siren.app_mapping_network(za)
            ends.append((trunc(avg_fg, fg), trunc(avg_fa, fa), trunc(avg_pg, pg), trunc(avg_pa, pa)))
    lerp = lambda a, b, t: a * (1 - t) + b * t
    frames, depths = [], []
    for i, t in enumerate(np.linspace(0, 1, n_frames)):
        t = float(t)
        if latent_type == "app":
            t = (t - 0.5) * 2
        move_geo, move_app = latent_type in ("geo", "both"), latent_type in ("app", "both")
        (fg1, fa1, pg1, pa1), (fg2, fa2, pg2, pa2) = ends
        film = (lerp(fg1, fg2, t) if move_geo else fg1, lerp(fa1, fa2, t) if move_app else fa1,
                lerp(pg1, pg2, t) if move_geo else pg1, lerp(pa1, pa2, t) if move_app else pa1)
        kw = dict(options)
        if trajectory is not None:
            kw["v_mean"], kw["h_mean"] = trajectory[i]
        img, depth, _ = generator.staged_forward_with_frequencies(*film, **kw)
        frames.append(img)
        depths.append(depth)
    return torch.cat(frames), torch.cat(depths)


# ---------------------------------------------------------------------------------------------------
# render_video_interpolation_semantic.py: options bag and camera trajectories
# ---------------------------------------------------------------------------------------------------
def video_kwargs(curriculum, image_size=256, ray_step_multiplier=2, psi=0.5, lock_view_dependence=False, num_frames=36, fov=12,
                 fill_color="black"):
    """The kwargs bag render_video_interpolation_semantic.py:52-69 builds from a curriculum."""
    c = dict(curriculum)
    c["num_steps"] = curriculum[0]["num_steps"] * ray_step_multiplier
    c["img_size"] = image_size
    c["psi"] = psi
    c["v_stddev"] = 0
    c["h_stddev"] = 0
    c["lock_view_dependence"] = lock_view_dependence
    c["last_back"] = curriculum.get("eval_last_back", False)
    c["num_frames"] = num_frames
    c["nerf_noise"] = 0
    c["fov"] = fov
    c["fill_mode"] = curriculum.get("fill_mode", "weight")
    if c["fill_mode"] == "seg_padding_background":
        c["fill_mode"] = "eval_seg_padding_background"
    c["fill_color"] = fill_color
    return {k: v for k, v in c.items() if type(k) is str}


def camera_trajectory(name, num_frames, fov):
    """[(t, pitch, yaw, fov)] of run_video_double_latent_interpolation (render_video_interpolation_semantic.py:326-379)."""
    pi = np.pi
    if name == "front":
        return [(t, 0.2 * np.cos(t * 2 * pi) + pi / 2, 0.4 * np.sin(t * 2 * pi) + pi / 2, fov + 5 + np.sin(t * 2 * pi) * 5)
                for t in np.linspace(0, 1, num_frames, endpoint=True)]
    if name == "orbit":
        return [(t, pi / 2, t * 2 * pi, fov) for t in np.linspace(0, 0.5, num_frames, endpoint=True)]
    if name == "rotation_horizontal":
        return [(t, pi / 2, pi / 2 + t * 0.5, fov) for t in np.linspace(-1, 1, num_frames)]
    if name == "non_rotation":
        return [(t, pi / 2, pi / 2, fov) for t in np.linspace(0, 1, num_frames, endpoint=True)]
    if name == "sphere":
        return [(t, 0.2 * np.cos(t * 2 * pi) + pi / 2, 0.4 * np.sin(t * 2 * pi) + pi / 2, fov) for t in np.linspace(0, 1, num_frames, endpoint=True)]
    if name == "zoom":
        return [(t, pi / 2, pi / 2, fov + np.sin(t * 2 * pi) * 5) for t in np.linspace(0, 1, num_frames)]
    raise ValueError(f"unknown trajectory {name!r} (front | orbit | rotation_horizontal | non_rotation | sphere | zoom)")


def render_double_latent_video(generator, seed, options, trajectory, latent_type="geo", psi=0.5, device=None, latents=None, geometry=False):
    """The frame loop of run_video_double_latent_interpolation (:381-430): two identities from seeds `seed` and `seed + 1`
    (z_geo then z_app each), FiLM parameters truncated towards the mean and interpolated on the `latent_type` side
    (DoubleFrequencyInterpolator, :130-176: 'app' sweeps t over [-1, 1]), one staged_forward_with_frequencies per trajectory
    entry with v_mean / h_mean / fov from it.  -> dict(images [F,3,S,S], labels [F,3,S,S] (0..255 colours), acc [F,3,S,S],
    depth [F,S,S]) on the CPU.  latents: optional ((z_geo1, z_app1), (z_geo2, z_app2)) instead of the seeded draws.
    geometry: True, or a dict of render_geometry's options -- every frame goes through render_geometry (the same render) and the dict
    gains normal [F,3,S,S] and shaded [F,1,S,S]; `acc` is then the weight sum * 2 - 1 whatever the fill_mode."""
    device = torch.device(device) if device is not None else generator.device
    zg_dim, za_dim = _latent_dims(generator)
    if latents is None:
        torch.manual_seed(seed)
        z1 = (torch.randn(1, zg_dim, device=device), torch.randn(1, za_dim, device=device))
        torch.manual_seed(int(seed) + 1)
        z2 = (torch.randn(1, zg_dim, device=device), torch.randn(1, za_dim, device=device))
    else:
        z1, z2 = (tuple(torch.as_tensor(t, dtype=torch.float32, device=device) for t in pair) for pair in latents)
    avg_fg, avg_pg, avg_fa, avg_pa = generator.generate_avg_frequencies()
    trunc = lambda avg, raw: avg + psi * (raw - avg)
    with torch.no_grad():
        ends = []
        for zg, za in (z1, z2):
            fg, pg = generator.siren.geo_mapping_network(zg)
            fa, pa = generator.siren.app_mapping_network(za)
            ends.append((trunc(avg_fg, fg), trunc(avg_fa, fa), trunc(avg_pg, pg), trunc(avg_pa, pa)))
    lerp = lambda a, b, t: a * (1 - t) + b * t
    (fg1, fa1, pg1, pa1), (fg2, fa2, pg2, pa2) = ends
    move_geo, move_app = latent_type in ("geo", "both"), latent_type in ("app", "both")
    out = dict(images=[], labels=[], acc=[], depth=[])
    geo = dict(geometry) if isinstance(geometry, dict) else {}
    if geometry:
        out.update(normal=[], shaded=[])
    kw = {k: v for k, v in options.items() if k != "num_frames"}
    for t, pitch, yaw, fov in trajectory:
        t = float(t)
        if latent_type == "app":
            t = (t - 0.5) * 2
        film = (lerp(fg1, fg2, t) if move_geo else fg1, lerp(fa1, fa2, t) if move_app else fa1,
                lerp(pg1, pg2, t) if move_geo else pg1, lerp(pa1, pa2, t) if move_app else pa1)
        kw.update(h_mean=float(yaw), v_mean=float(pitch), fov=float(fov), h_stddev=0, v_stddev=0)
        if geometry:
            meta = dict(truncated_frequencies_geo=film[0], truncated_frequencies_app=film[1], truncated_phase_shifts_geo=film[2], truncated_phase_shifts_app=film[3])
            view = render_geometry(generator, film=meta, **geo, **kw)
            frame, depth = view["pixels"], view["depth"]
            weight_sum = (view["alpha"] * 2 - 1)[:, None].expand(-1, 3, -1, -1)
            out["normal"].append(view["normal"])
            out["shaded"].append(view["shaded"])
        else:
            frame, depth, weight_sum = generator.staged_forward_with_frequencies(*film, **kw)
        out["images"].append(frame[:, -3:])
        out["labels"].append(mask2color(frame[:, :-3], device))
        out["acc"].append(weight_sum[:, -3:])
        out["depth"].append(depth)
    return {k: torch.cat(v) for k, v in out.items()}


def camera_trajectory_single(name, num_frames, fov):
    """[(t, pitch, yaw, fov)] of run_video_latent_interpolation, the single-latent variant (render_video_interpolation_semantic.py:
    197-262) -- its 'orbit' and 'rotation_horizontal' differ from the double-latent function's, and it has 'rotation_angles' /
    'rotation_pi' instead of 'zoom'."""
    pi = np.pi
    lin = lambda a, b, n: np.linspace(a, b, n)
    if name == "front":
        return [(t, 0.2 * np.cos(t * 2 * pi) + pi / 2, 0.4 * np.sin(t * 2 * pi) + pi / 2, fov + 5 + np.sin(t * 2 * pi) * 5) for t in lin(0, 1, num_frames)]
    if name == "orbit":
        return [(t, 0.2 * np.cos(t * 2 * pi) + pi / 4, t * 2 * pi, fov) for t in lin(0, 1, num_frames)]
    if name == "rotation_horizontal":
        return [(t, pi / 2, pi / 2 + t * 0.5, fov) for t in list(lin(-1, 1, num_frames // 2)) + list(lin(1, -1, num_frames // 2))]
    if name == "rotation_angles":
        return [(t, pi / 2, pi / 2 + a, fov) for t, a in enumerate([-0.5, -0.25, 0.0, 0.25, 0.5])]
    if name == "rotation_pi":
        return [(t, pi / 2, pi / 2 + t * 0.5 * pi, fov) for t in lin(-1, 1, num_frames)]
    if name == "non_rotation":
        return [(t, pi / 2, pi / 2, fov) for t in lin(0, 1, num_frames)]
    if name == "sphere":
        return [(t, 0.2 * np.cos(t * 2 * pi) + pi / 2, 0.4 * np.sin(t * 2 * pi) + pi / 2, fov) for t in lin(0, 1, num_frames)]
    raise ValueError(f"unknown trajectory {name!r} (front | orbit | rotation_horizontal | rotation_angles | rotation_pi | non_rotation | sphere)")


def render_latent_video(generator, seed, options, trajectory, latent_type="geo", psi=0.5, device=None, latents=None):
    """The frame loop of run_video_latent_interpolation (:264-299) for a single-latent ImplicitGenerator3d: z_current, z_next drawn
    back to back after torch.manual_seed(seed), FiLM parameters truncated towards the mean (FrequencyInterpolator, :109-128) and
    interpolated with the trajectory's t (latent_type 'non': the first identity throughout), one
    staged_forward_with_frequencies per trajectory entry.  -> dict(images [F,C,S,S] on the device, depth [F,S,S] on the CPU)."""
    device = torch.device(device) if device is not None else generator.device
    z_dim = int(getattr(generator, "z_dim", 256))
    if latents is None:
        torch.manual_seed(seed)
        z1 = torch.randn(1, z_dim, device=device)
        z2 = torch.randn(1, z_dim, device=device)
    else:
        z1, z2 = (torch.as_tensor(t, dtype=torch.float32, device=device) for t in latents)
    avg_f, avg_p = generator.generate_avg_frequencies()
    with torch.no_grad():
        f1, p1 = generator.siren.mapping_network(z1)
        f2, p2 = generator.siren.mapping_network(z2)
    f1, p1, f2, p2 = avg_f + psi * (f1 - avg_f), avg_p + psi * (p1 - avg_p), avg_f + psi * (f2 - avg_f), avg_p + psi * (p2 - avg_p)
    out = dict(images=[], depth=[])
    kw = {k: v for k, v in options.items() if k != "num_frames"}
    for t, pitch, yaw, fov in trajectory:
        t = float(t)
        film = (f1, p1) if latent_type == "non" else (f1 * (1 - t) + f2 * t, p1 * (1 - t) + p2 * t)
        kw.update(h_mean=float(yaw), v_mean=float(pitch), fov=float(fov), h_stddev=0, v_stddev=0)
        frame, depth = generator.staged_forward_with_frequencies(*film, **kw)
        out["images"].append(frame)
        out["depth"].append(depth)
    return {k: torch.cat(v) for k, v in out.items()}



# ------------------------------------------------------------------------------------------------------------------------------------
# The image dump of the reference's FID evaluation (fid_evaluation.py:96-150), which is how its forward path runs on several GPUs:
# every rank renders batches of 4 identities with staged_forward and writes the images whose ids are rank, rank + world, ... -- no
# data-path collective (the FID statistics themselves are third-party code on the dumped files and are not part of this package).
# ------------------------------------------------------------------------------------------------------------------------------------
def fid_dump_metadata(input_metadata, img_size=128, batch_size=4):
    """The option bag both dump loops build from the training step's metadata (fid_evaluation.py:97-106, :127-135): 128 x 128, batches
    of 4, the *_eval pose spread / distribution when the curriculum has them, psi = 1."""
    import copy
    metadata = copy.deepcopy(dict(input_metadata))
    metadata['img_size'] = img_size
    metadata['batch_size'] = batch_size
    metadata['h_stddev'] = metadata.get('h_stddev_eval', metadata['h_stddev'])
    metadata['v_stddev'] = metadata.get('v_stddev_eval', metadata['v_stddev'])
    metadata['sample_dist'] = metadata.get('sample_dist_eval', metadata['sample_dist'])
    metadata['psi'] = 1
    return metadata


class _OrderedWriter:
    """save(img, path) calls on ONE worker thread, in submission order: the JPEG encoding of a batch runs while the device renders the next
    one (the reference writes between renders, fid_evaluation.py:115-121; same files, same order).  An exception of `save` is raised by
    the next submit() or by close()."""

    def __init__(self, save):
        from concurrent.futures import ThreadPoolExecutor
        self.save, self.pool, self.pending = save, ThreadPoolExecutor(max_workers=1), []

    def _reap(self, wait):
        while self.pending and (wait or self.pending[0].done()):
            self.pending.pop(0).result()

    def submit(self, img, path):
        self._reap(False)
        self.pending.append(self.pool.submit(self.save, img, path))

    def close(self):
        try:
            self._reap(True)
        finally:
            self.pool.shutdown(wait=True)


def _dump_loop(generator, metadata, rank, world_size, output_dir, num_imgs, draw, save):
    import os
    from . import imageio_lite
    module = getattr(generator, "module", generator)        # the reference passes the DistributedDataParallel wrapper
    os.makedirs(output_dir, exist_ok=True)
    save = save or (lambda img, path: imageio_lite.save_image(img, path, normalize=True, value_range=(-1, 1)))
    generator.eval()
    img_counter = rank
    written = []
    writer = _OrderedWriter(save)
    try:
        with torch.no_grad():
            while img_counter < num_imgs:
                generated_imgs = draw(module, metadata)
                for img in generated_imgs:          # (a batch is written out whole: the last one may run past num_imgs, as in the reference)
                    if img.shape[0] != 3:
                        img = img[-3:]
                    path = os.path.join(output_dir, f'{img_counter:0>5}.jpg')
                    writer.submit(img, path)
                    written.append(path)
                    img_counter += world_size
    finally:
        writer.close()
    return written


def output_images(generator, input_metadata, rank, world_size, output_dir, num_imgs=2048, save=None):
    """fid_evaluation.output_images (:96-123) for the single-latent generators: z ~ randn [4, z_dim] per batch,
    staged_forward(z, **metadata)[0], image ids rank, rank + world_size, ... as `<id:05>.jpg` normalised from [-1, 1].
    -> the paths this rank wrote.  `save(img [3,S,S], path)` replaces the writer (tests)."""
    metadata = fid_dump_metadata(input_metadata)

    def draw(module, md):
        z = torch.randn((md['batch_size'], module.z_dim), device=module.device)
        return module.staged_forward(z, **md)[0]
    return _dump_loop(generator, metadata, rank, world_size, output_dir, num_imgs, draw, save)


def output_images_double(generator, input_metadata, rank, world_size, output_dir, num_imgs=2048, save=None):
    """fid_evaluation.output_images_double (:126-150) for the two-latent generators: z_geo then z_app ~ randn [4, dim] per batch,
    staged_forward(z_geo, z_app, **metadata)[0], the last three channels (rgb) of every image, ids rank, rank + world_size, ..."""
    metadata = fid_dump_metadata(input_metadata)

    def draw(module, md):
        z_geo = torch.randn((md['batch_size'], module.z_geo_dim), device=module.device)
        z_app = torch.randn((md['batch_size'], module.z_app_dim), device=module.device)
        return module.staged_forward(z_geo, z_app, **md)[0]
    return _dump_loop(generator, metadata, rank, world_size, output_dir, num_imgs, draw, save)


def eval_metrics_images(generator, curriculum, output_dir, num_images=2048, max_batch_size=94800000, save=None):
    """The image loop of the reference's eval_metrics.py (:41-52; single-latent generators): render options = the curriculum stage of
    `generator.step` with img_size 128, psi 1, last_back = eval_last_back, nerf_noise 0; one identity per call, z ~ randn [1, latent_dim],
    staged_forward(z, max_batch_size=..., **options)[0] written as `<i:05>.jpg` normalised from [-1, 1].  (The script then hands the
    directory to torch_fidelity -- third-party, not part of this package.)  -> the paths written."""
    import os
    from . import curriculums as _cur, imageio_lite
    options = _cur.extract_metadata(curriculum, generator.step)
    options['img_size'] = 128
    options['psi'] = 1
    options['last_back'] = options.get('eval_last_back', False)
    options['nerf_noise'] = 0
    os.makedirs(output_dir, exist_ok=True)
    save = save or (lambda img, path: imageio_lite.save_image(img, path, normalize=True, value_range=(-1, 1)))
    generator.eval()
    written = []
    writer = _OrderedWriter(save)
    try:
        for img_counter in range(num_images):
            z = torch.randn(1, options['latent_dim'], device=generator.device)
            with torch.no_grad():
                img = generator.staged_forward(z, max_batch_size=max_batch_size, **options)[0].to(generator.device)
            path = os.path.join(output_dir, f'{img_counter:0>5}.jpg')
            writer.submit(img, path)
            written.append(path)
    finally:
        writer.close()
    return written


def training_snapshots(generator, ema, fixed_z_geo, fixed_z_app, metadata, output_dir, step, device=None):
    """The sample-image block of the reference's training loop (train_double_latent_semantic.py:464-523), which is how staged_forward is
    called DURING training: under autocast, 25 fixed identities at 128 x 128 with the pose spread at zero, frontal and tilted
    (h_mean + 0.5), with the live weights and again with the EMA weights swapped in (store / copy_to / eval ... restore), plus 25 fresh
    identities at psi = 0.7 under the EMA weights.  Writes `<step>_{seg,img}_{fixed,tilted,fixed_ema,tilted_ema,random}.png`
    (5 x 5 grids, normalised over the batch like torchvision's save_image(normalize=True)) -> their paths.
    `generator`: the module or its DistributedDataParallel wrapper; `ema`: a torch_ema.ExponentialMovingAverage (or fenerf_amd.ema's)."""
    import copy
    import os
    from . import imageio_lite
    module = getattr(generator, "module", generator)
    device = module.device if device is None else device
    os.makedirs(output_dir, exist_ok=True)
    written = []

    def dump(tag, z_geo, z_app, **overrides):
        with torch.no_grad():
            with torch.autocast("cuda", enabled=torch.device(device).type == "cuda"):
                copied_metadata = copy.deepcopy(metadata)
                copied_metadata['h_stddev'] = copied_metadata['v_stddev'] = 0
                copied_metadata['img_size'] = 128
                for k, v in overrides.items():
                    copied_metadata[k] = copied_metadata[k] + v if k == 'h_mean' else v
                gen_imgs = module.staged_forward(z_geo.to(device), z_app.to(device), **copied_metadata)[0]
                gen_labels = mask2color(gen_imgs[:, :-3], device)
        for kind, t in (("seg", gen_labels[:25]), ("img", gen_imgs[:25, -3:])):
            path = os.path.join(output_dir, f"{step}_{kind}_{tag}.png")
            imageio_lite.save_image(t, path, nrow=5, normalize=True)
            written.append(path)

    generator.eval()
    dump("fixed", fixed_z_geo, fixed_z_app)
    dump("tilted", fixed_z_geo, fixed_z_app, h_mean=0.5)
    ema.store(generator.parameters())
    ema.copy_to(generator.parameters())
    generator.eval()
    dump("fixed_ema", fixed_z_geo, fixed_z_app)
    dump("tilted_ema", fixed_z_geo, fixed_z_app, h_mean=0.5)
    dump("random", torch.randn_like(fixed_z_geo), torch.randn_like(fixed_z_app), psi=0.7)
    ema.restore(generator.parameters())
    return written
