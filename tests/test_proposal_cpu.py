"""Host side of the proposal lattice (a render's samples placed from a baked density lattice): the declarations, the workspace size, the
command-line options and the argument refusals that need no device.  Nothing here touches the kernels."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fenerf_amd import _lib, callers, native  # noqa: E402

ENTRIES = ("fenerf_proposal_depths", "fenerf_render_proposal_workspace_bytes", "fenerf_render_proposal")


def test_entries_are_declared_exported_and_on_the_library():
    hdr = open(os.path.join(ROOT, "include", "fenerf.h")).read()
    l = _lib.lib()
    for name in ENTRIES:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\(([^;]*?)\);", hdr, re.S)
        assert m, name
        n_args = len([a for a in m.group(2).split(",") if a.strip()])
        res, args = _lib._SIGS[name]
        assert name in _lib.EXPORTS and hasattr(l, name) and len(args) == n_args, (name, len(args), n_args)
        assert res is (_lib._sz if m.group(1) == "size_t" else _lib._i)
    # the size argument of the render sits where the header has it
    assert _lib._SIGS["fenerf_render_proposal"][1][-2] is _lib._sz
    assert "#define FENERF_ABI_VERSION 2" in hdr and "#define FENERF_N_PHASES 17" in hdr
    assert l.fenerf_abi_version() == 2 and _lib.ABI_VERSION == 2
    for f in (native.proposal_depths, native.NativeModel.render_proposal, callers.bake_density, callers.DensityField.sample, callers.DensityField.render):
        assert callable(f)


def test_workspace_is_the_fine_depths_and_the_rows():
    size = _lib.lib().fenerf_render_proposal_workspace_bytes
    for B, R, N, C_ in ((2, 16, 12, 22), (1, 3, 3, 4), (1, 65536, 48, 22), (1, 1, 512, 2)):
        pts = B * R * N
        want = pts * 4 + pts * C_ * 4               # z_fine + [B*R][N][C] rows
        assert want <= size(B, R, N, C_) <= want + 2 * 256, (B, R, N, C_)
    for bad in ((0, 16, 12, 22), (2, 0, 12, 22), (-1, 16, 12, 22), (2, 16, 2, 22), (2, 16, 513, 22), (2, 16, 12, 1), (2, 16, 12, 65)):
        assert size(*bad) == 0, bad


def test_both_parsers_take_proposal_and_refuse_the_other_routes(capsys):
    import inverse_render
    import render_multiview
    assert render_multiview.build_parser().parse_args(["g.pth"]).proposal is None
    assert render_multiview.parse_options(["g.pth"]).proposal is None
    opt = render_multiview.parse_options(["g.pth", "--proposal", "128"])
    assert opt.proposal == 128 and opt.baked is None and not opt.labels_only and not opt.geometry
    for other in (["--baked", "64"], ["--labels_only"], ["--geometry"]):
        with pytest.raises(SystemExit):
            render_multiview.parse_options(["g.pth", "--proposal", "128"] + other)
        assert "--proposal" in capsys.readouterr().err
    assert inverse_render.build_parser().parse_args(["n", "g.pth"]).proposal is None
    assert inverse_render.parse_options(["n", "g.pth"]).proposal is None
    assert inverse_render.parse_options(["n", "g.pth", "--recon", "--proposal", "128"]).proposal == 128
    with pytest.raises(SystemExit):
        inverse_render.parse_options(["n", "g.pth", "--recon", "--proposal", "128", "--baked", "64"])
    assert "--proposal" in capsys.readouterr().err


def test_the_tool_hands_proposal_to_the_caller(monkeypatch, tmp_path):
    import render_multiview as tool
    seen = {}

    def fake_render_multiview(generator, curriculum, seed, device, **kw):
        seen.update(kw)
        return torch.zeros((5, 3, 8, 8)), torch.zeros((5, 3, 8, 8))

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(callers, "load_generator", lambda *a, **k: object())
    monkeypatch.setattr(callers, "render_multiview", fake_render_multiview)
    tool.main(["gen.pth", "--proposal", "33", "--image_size", "8", "--output_dir", str(tmp_path)])
    assert seen["proposal"] == 33 and seen["baked"] is None and seen["geometry"] is False
    tool.main(["gen.pth", "--image_size", "8", "--output_dir", str(tmp_path)])
    assert seen["proposal"] is None                       # the default: the exact renders


CUR = {0: dict(num_steps=3), "h_mean": 0.0}


def test_callers_refuse_proposal_with_the_other_routes():
    for other in (dict(baked=9), dict(labels_only=True), dict(geometry=True), dict(geometry=dict(ambient=0.1))):
        with pytest.raises(ValueError, match="proposal"):
            callers.render_multiview(None, CUR, 0, "cpu", proposal=9, **other)
    with pytest.raises(ValueError, match="at least 2"):
        callers.render_multiview(None, CUR, 0, "cpu", proposal=1)
    with pytest.raises(ValueError, match="proposal"):
        callers.render_inversion_views(None, {}, {}, proposal=9, baked=9)
    with pytest.raises(ValueError, match="proposal"):
        callers.render_inversion_recon(None, {}, {}, [], proposal=9, baked=9)


class _Gen:
    device = "cpu"
    siren = None


def test_bake_density_and_render_refusals_that_need_no_device():
    f = torch.zeros((1, 4))
    meta = dict(truncated_frequencies_geo=f, truncated_phase_shifts_geo=f, truncated_frequencies_app=f, truncated_phase_shifts_app=f)
    with pytest.raises(ValueError, match="at least 2"):
        callers.bake_density(_Gen(), None, film=meta, resolution=1, cube_length=1.0)
    with pytest.raises(RuntimeError, match="no-grad"):
        callers.bake_density(_Gen(), None, film=dict(meta, truncated_phase_shifts_geo=f.clone().requires_grad_(True)), resolution=5, cube_length=1.0)
    two = torch.zeros((2, 4))
    with pytest.raises(ValueError, match="one identity"):
        callers.bake_density(_Gen(), None, film={k: two for k in meta}, resolution=5, cube_length=1.0)
    with pytest.raises(TypeError):
        callers.bake_density(_Gen(), None, film=meta, resolution=5)              # cube_length has no default
    field = callers.DensityField(torch.zeros((2, 2, 2)), (0, 0, 0), (1, 1, 1), (f, f, f, f))
    assert field.outside_last == callers.BAKED_OUTSIDE_SIGMA
    kw = dict(img_size=4, fov=12, ray_start=0.88, ray_end=1.12, num_steps=6, h_stddev=0.0, v_stddev=0.0, h_mean=1.5, v_mean=1.5)
    with pytest.raises(ValueError, match="hierarchical_sample"):
        field.render(_Gen(), hierarchical_sample=False, **kw)
    g_field = callers.DensityField(field.vol, field.origin, field.spacing, (f.clone().requires_grad_(True), f, f, f))
    with pytest.raises(RuntimeError, match="no-grad"):
        g_field.render(_Gen(), **kw)
    with pytest.raises(RuntimeError, match="no-grad"):
        field.render(_Gen(), **dict(kw, h_mean=torch.tensor(1.5, requires_grad=True)))
    with pytest.raises(RuntimeError, match="no-grad"):
        field.sample(torch.zeros((3, 3), requires_grad=True))
