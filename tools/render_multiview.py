#!/usr/bin/env python
"""Multi-view renders of a trained generator on the MI355X-native path -- the command-line surface of the reference's
render_multiview_images_double_semantic.py (:31-42), same positional argument and options:

    python tools/render_multiview.py <path/to/generator.pth> --curriculum CelebA_double_semantic_texture_embedding_256_dim_96 \\
           --seeds 0 1 2 --output_dir imgs [--image_size 256] [--ray_step_multiplier 2] [--lock_view_dependence] [--max_batch_size N]

For every seed: five yaw angles (-0.5 .. 0.5 rad around h_mean) of the identity drawn from `torch.manual_seed(seed)`, written as
`grid_<seed>_RGB.png` (normalised from [-1, 1]) and `grid_<seed>_SEG.png` (argmax -> colour LUT, already in [0, 1]) with
torchvision.save_image's grid layout.  `<prefix>ema.pth` next to the generator pickle is loaded and copied in, as the reference
does (:61-64).  `--max_batch_size` is accepted and ignored: the fused renderer never materialises per-point activations.
(The reference's SEG line passes the misspelt `noralize=True`, which torchvision 0.9's save_image rejects; the colour maps are
in [0, 1] already, so this writes them unnormalised -- what that line means.)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('path', type=str)
    parser.add_argument('--seeds', nargs='+', default=[0])
    parser.add_argument('--output_dir', type=str, default='imgs')
    parser.add_argument('--max_batch_size', type=int, default=2400000)
    parser.add_argument('--lock_view_dependence', action='store_true')
    parser.add_argument('--image_size', type=int, default=256)
    parser.add_argument('--ray_step_multiplier', type=int, default=2)
    parser.add_argument('--curriculum', type=str, default='CelebA')
    parser.add_argument('--no_ema', action='store_true', help='render the raw generator weights (not in the reference: it always loads <prefix>ema.pth)')
    parser.add_argument('--baked', type=int, default=None, metavar='RES',
                        help='bake each identity once into a RES^3 lattice (view direction locked) and render its views by trilinear lookup: an '
                             'approximation, RES^3 x 96 bytes of device memory (not in the reference; default: the exact renders)')
    parser.add_argument('--labels_only', action='store_true',
                        help='render only the semantic row (grid_<seed>_SEG.png, the same pixels) through the density route: no colour branch, no '
                             'RGB grid (not in the reference; not with --baked or --geometry)')
    parser.add_argument('--proposal', type=int, default=None, metavar='RES',
                        help='bake each identity\'s density once into a RES^3 lattice and place every view\'s samples from it: one SIREN pass per '
                             'view at the resampled depths, view-dependent colour kept; approximates sample placement only, RES^3 x 4 bytes of '
                             'device memory (not in the reference; not with --baked, --labels_only or --geometry)')
    parser.add_argument('--roll', type=float, default=None, metavar='DEG',
                        help='roll every view by DEG degrees about its view axis (a free camera, fenerf_amd.camera; not in the reference)')
    parser.add_argument('--radius', type=float, default=None, metavar='X',
                        help='camera distance from the origin (the reference: 1; a free camera)')
    parser.add_argument('--crop', type=int, nargs=4, default=None, metavar=('X0', 'Y0', 'W', 'H'),
                        help='render only this window of every --image_size view (a free camera)')
    add_geometry_arguments(parser)
    return parser


def parse_options(argv=None):
    """the parsed arguments, with the combinations no route serves refused by the parser"""
    parser = build_parser()
    opt = parser.parse_args(argv)
    if opt.labels_only and (opt.baked is not None or opt.geometry):
        parser.error("--labels_only takes neither --baked nor --geometry")
    if opt.proposal is not None and (opt.baked is not None or opt.labels_only or opt.geometry):
        parser.error("--proposal places the samples of the exact colour render; it takes none of --baked, --labels_only, --geometry")
    if uses_camera(opt) and (opt.baked is not None or opt.labels_only or opt.geometry or opt.proposal is not None):
        parser.error("--roll / --radius / --crop render the exact colour views; they take none of --baked, --labels_only, --geometry, --proposal")
    if opt.crop is not None:
        x0, y0, w, h = opt.crop
        if x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > opt.image_size or y0 + h > opt.image_size:
            parser.error(f"--crop {x0} {y0} {w} {h} is empty or lies outside the {opt.image_size} x {opt.image_size} image")
    if opt.radius is not None and not opt.radius > 0:
        parser.error("--radius must be positive")
    return opt


def uses_camera(opt):
    return opt.roll is not None or opt.radius is not None or opt.crop is not None


FACE_ANGLES = (-0.5, -0.25, 0.0, 0.25, 0.5)


def view_cameras(opt, curriculum, device):
    """the five views of render_multiview as free cameras with the flags' roll, radius and window"""
    import math
    from fenerf_amd.camera import Camera
    cams = []
    for a in FACE_ANGLES:
        cam = Camera.from_angles(a + curriculum['h_mean'], curriculum['v_mean'], curriculum['fov'], (opt.image_size, opt.image_size),
                                 radius=1.0 if opt.radius is None else opt.radius, roll=math.radians(opt.roll or 0.0), device=device)
        cams.append(cam if opt.crop is None else cam.crop(*opt.crop))
    return cams


def add_geometry_arguments(parser):
    parser.add_argument('--geometry', action='store_true',
                        help='also write the normal map (n * 0.5 + 0.5) and the Lambert-shaded shape image of every view, as <name>_normal / '
                             '<name>_shaded (callers.render_geometry; not in the reference).  Combines with --baked: lattice normals')
    parser.add_argument('--light', type=float, nargs=3, default=(0.0, 0.0, 1.0), metavar=('X', 'Y', 'Z'), help='light direction in camera space (--geometry)')
    parser.add_argument('--ambient', type=float, default=0.25, help='ambient term of the shaded image (--geometry)')


def geometry_options(opt):
    """render_multiview's / render_double_latent_video's `geometry` argument from the flags above"""
    return dict(light=tuple(opt.light), ambient=opt.ambient) if opt.geometry else False


def resolve_curriculum(name):
    """A curriculum of fenerf_amd.curriculums by name (the reference's behaviour), or -- an extension for tests and custom
    models -- a JSON file in tests/golden/curriculums.json's spelling (integer stage keys as "int:<step>")."""
    import json
    from fenerf_amd import curriculums
    if hasattr(curriculums, name):
        return dict(getattr(curriculums, name))
    if os.path.isfile(name):
        d = json.load(open(name))
        return {(int(k[4:]) if k.startswith("int:") else k): v for k, v in d.items()}
    raise SystemExit(f"unknown curriculum {name!r}")


def main(argv=None):
    from fenerf_amd import host
    host.respect_cpu_quota()          # torch's CPU thread pool no larger than the cores this process is granted (fenerf_amd/host.py)
    opt = parse_options(argv)
    import torch
    from fenerf_amd import callers, imageio_lite
    if not torch.cuda.is_available():
        raise SystemExit("render_multiview.py renders on the GPU (fenerf_amd has no CPU path)")
    device = torch.device('cuda')
    curriculum = resolve_curriculum(opt.curriculum)
    os.makedirs(opt.output_dir, exist_ok=True)
    generator = callers.load_generator(opt.path, device, use_ema=not opt.no_ema)
    for seed in opt.seeds:
        if opt.labels_only:
            segmaps, _ = callers.render_multiview(generator, curriculum, int(seed), device, image_size=opt.image_size,
                                                  ray_step_multiplier=opt.ray_step_multiplier, lock_view_dependence=opt.lock_view_dependence,
                                                  labels_only=True)
            imageio_lite.save_image(segmaps, os.path.join(opt.output_dir, f'grid_{seed}_SEG.png'))
            print(f"seed {seed}: {tuple(segmaps.shape)} -> {opt.output_dir}/grid_{seed}_SEG.png")
            continue
        images, segmaps, *views = callers.render_multiview(generator, curriculum, int(seed), device, image_size=opt.image_size,
                                                           ray_step_multiplier=opt.ray_step_multiplier,
                                                           lock_view_dependence=opt.lock_view_dependence, baked=opt.baked,
                                                           geometry=geometry_options(opt), proposal=opt.proposal,
                                                           cameras=view_cameras(opt, curriculum, device) if uses_camera(opt) else None)
        imageio_lite.save_image(images, os.path.join(opt.output_dir, f'grid_{seed}_RGB.png'), normalize=True, value_range=(-1, 1))
        imageio_lite.save_image(segmaps, os.path.join(opt.output_dir, f'grid_{seed}_SEG.png'))
        if views:
            normals, shaded = views
            imageio_lite.save_image(normals * 0.5 + 0.5, os.path.join(opt.output_dir, f'grid_{seed}_normal.png'))
            imageio_lite.save_image(shaded, os.path.join(opt.output_dir, f'grid_{seed}_shaded.png'))
        print(f"seed {seed}: {tuple(images.shape)} -> {opt.output_dir}/grid_{seed}_RGB.png, grid_{seed}_SEG.png")


if __name__ == '__main__':
    main()
