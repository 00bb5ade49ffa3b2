#!/usr/bin/env python
"""Density volumes for shape extraction on the MI355X-native path -- the command-line surface of the reference's
extract_double_semantic_shapes.py (:89-139; extract_shapes.py is its single-latent twin), same positional argument and options:

    python tools/extract_shapes.py <path/to/generator.pth> --seeds 3 4 5 --cube_size 0.3 --voxel_resolution 256 --output_dir shapes
    python tools/extract_shapes.py <path/to/generator.pth> --latent_path <save_dir>/freq_phase_offset_<name>.pth --seeds 7

Without --latent_path: for every seed the identity z = randn(1, z_dim) under torch.manual_seed(seed) (the script feeds the same z to both
mapping networks), FiLM parameters truncated towards the mean with psi = 0.5, sigma evaluated on the voxel_resolution^3 lattice of a
cube of side --cube_size with the view direction locked to (0, 0, -1) -> <output_dir>/<seed>.mrc.  With --latent_path: the identity of
an inversion checkpoint (mean + offsets; tools/inverse_render.py or the reference's script wrote it) -> <output_dir>/<seeds[0]>.mrc.
All N^3 points go through ONE fused SIREN launch (the reference walks them in chunks of 24,000 / 100,000).  The volume is written as an
MRC2014 mode-2 map by fenerf_amd.imageio_lite.write_mrc (mrcfile is not a dependency); marching cubes on it is the downstream step
the reference also leaves to other tools (skimage.measure + plyfile).  With --mesh that step runs here, on the device:
callers.extract_mesh (marching tetrahedra at the density level --iso, default 10; labels, colours and normals from the SIREN at the
vertices) -> <output_dir>/<seed>.ply beside the .mrc.  `<prefix>ema.pth` next to the generator pickle is loaded and copied in (:103-104).

    python tools/extract_shapes.py <path/to/generator.pth> --seeds 3 --mesh --iso 10
    python tools/extract_shapes.py <path/to/generator.pth> --seeds 3 --mesh --keep_largest --simplify 2

--keep_largest / --min_component N drop detached blobs of density before meshing (only the largest connected component of
{sigma >= iso}, or every component of at least N lattice points, stays); --simplify K merges the vertices of every K^3 block of cells
(vertex clustering) before labels, colours and normals are evaluated.  All three are off by default and need --mesh.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('path', type=str)
    parser.add_argument('--seeds', nargs='+', default=[3, 4, 5])
    parser.add_argument('--cube_size', type=float, default=0.3)
    parser.add_argument('--voxel_resolution', type=int, default=256)
    parser.add_argument('--output_dir', type=str, default='shapes')
    parser.add_argument('--latent_path', type=str, default=None)
    parser.add_argument('--no_ema', action='store_true', help='use the raw generator weights (not in the reference: it always loads <prefix>ema.pth)')
    parser.add_argument('--mesh', action='store_true', help='also write <seed>.ply: the labelled, coloured iso-surface (not in the reference)')
    parser.add_argument('--iso', type=float, default=10.0, help='density level of the --mesh surface')
    parser.add_argument('--keep_largest', action='store_true', help='--mesh: keep only the largest connected component of {sigma >= iso}')
    parser.add_argument('--min_component', type=int, default=None, metavar='N', help='--mesh: drop components of fewer than N lattice points')
    parser.add_argument('--labels', action='store_true',
                        help='also write <seed>_labels.npy beside the .mrc: the semantic class (argmax of the label logits, uint8) of every lattice point '
                             '(not in the reference)')
    parser.add_argument('--simplify', type=int, default=None, metavar='K', help='--mesh: merge the vertices of every K^3 block of cells (K >= 2)')
    return parser


def mesh_options(opt):
    """the keep= / simplify= arguments of callers.extract_mesh the flags ask for"""
    if opt.keep_largest and opt.min_component is not None:
        raise SystemExit("--keep_largest and --min_component exclude each other")
    if opt.min_component is not None and opt.min_component < 1:
        raise SystemExit("--min_component needs N >= 1")
    if opt.simplify is not None and opt.simplify < 2:
        raise SystemExit("--simplify needs K >= 2")
    keep = "largest" if opt.keep_largest else (opt.min_component if opt.min_component is not None else "all")
    return dict(keep=keep, simplify=opt.simplify)


def sample_volume(sample, opt, *args, **kwargs):
    """(density volume, label volume or None) of callers.sample_generator / sample_generator_wth_frequencies_phase_shifts as --labels asks"""
    if opt.labels:
        return sample(*args, return_labels=True, **kwargs)
    return sample(*args, **kwargs), None


def write_labels(path, labels):
    import numpy as np
    np.save(path, labels)
    print(f"  labels {labels.shape} uint8, {len(np.unique(labels))} classes present -> {path}")


def write_mesh(callers, imageio_lite, path, generator, opt, **latent):
    mesh = callers.extract_mesh(generator, latent.pop('z', None), cube_length=opt.cube_size, voxel_resolution=opt.voxel_resolution, iso=opt.iso,
                                **mesh_options(opt), **latent)
    imageio_lite.write_ply(path, mesh['vertices'], mesh['faces'], normal=mesh['normal'], rgb=mesh['rgb'], label=mesh['label'])
    cleaned = f" ({mesh['components']} components before filtering)" if 'components' in mesh else ""
    print(f"  mesh at sigma = {opt.iso:g}: {len(mesh['vertices'])} vertices, {len(mesh['faces'])} faces{cleaned} -> {path}")


def main(argv=None):
    from fenerf_amd import host
    host.respect_cpu_quota()          # torch's CPU thread pool no larger than the cores this process is granted (fenerf_amd/host.py)
    opt = build_parser().parse_args(argv)
    import torch
    from fenerf_amd import callers, imageio_lite
    if not torch.cuda.is_available():
        raise SystemExit("extract_shapes.py evaluates on the GPU (fenerf_amd has no CPU path)")
    device = torch.device('cuda')
    generator = callers.load_generator(opt.path, device, use_ema=not opt.no_ema)
    os.makedirs(opt.output_dir, exist_ok=True)
    if opt.latent_path is None:
        z_dim = callers._latent_dims(generator)[0]
        for seed in opt.seeds:
            torch.manual_seed(int(seed))
            z = torch.randn(1, z_dim, device=device)
            voxel_grid, labels = sample_volume(callers.sample_generator, opt, generator, z, cube_length=opt.cube_size,
                                               voxel_resolution=opt.voxel_resolution)
            out = os.path.join(opt.output_dir, f'{seed}.mrc')
            imageio_lite.write_mrc(out, voxel_grid)
            if labels is not None:
                write_labels(os.path.join(opt.output_dir, f'{seed}_labels.npy'), labels)
            print(f"seed {seed}: sigma {voxel_grid.shape} in [{voxel_grid.min():.3g}, {voxel_grid.max():.3g}] -> {out}")
            if opt.mesh:
                # the mean FiLM parameters are drawn from the generator state the seed and the z draw leave behind: the same state again, so
                # that the surface is the level set of the volume just written
                torch.manual_seed(int(seed))
                z = torch.randn(1, z_dim, device=device)
                write_mesh(callers, imageio_lite, os.path.join(opt.output_dir, f'{seed}.ply'), generator, opt, z=z)
    else:
        meta = torch.load(opt.latent_path, map_location=device, weights_only=False)
        fg, fa, pg, pa = callers.film_from_inversion(meta, device)
        meta = dict(meta, truncated_frequencies_geo=fg, truncated_frequencies_app=fa, truncated_phase_shifts_geo=pg, truncated_phase_shifts_app=pa)
        voxel_grid, labels = sample_volume(callers.sample_generator_wth_frequencies_phase_shifts, opt, generator, meta, cube_length=opt.cube_size,
                                           voxel_resolution=opt.voxel_resolution)
        out = os.path.join(opt.output_dir, f'{opt.seeds[0]}.mrc')
        imageio_lite.write_mrc(out, voxel_grid)
        if labels is not None:
            write_labels(os.path.join(opt.output_dir, f'{opt.seeds[0]}_labels.npy'), labels)
        if opt.mesh:
            write_mesh(callers, imageio_lite, os.path.join(opt.output_dir, f'{opt.seeds[0]}.ply'), generator, opt, film=meta)
        print(f"inverted identity {opt.latent_path}: sigma {voxel_grid.shape} in [{voxel_grid.min():.3g}, {voxel_grid.max():.3g}] -> {out}")


if __name__ == '__main__':
    main()
