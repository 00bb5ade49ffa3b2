"""Host logic of the geometry route (density and labels without the colour branch): the command-line options parse and reach the callers,
the callers choose between the density query and the full forward by what the model says, and _lib declares the new entries with the
header's argument counts.  No GPU: the model objects are stubs."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fenerf_amd import _lib, callers  # noqa: E402

ENTRIES = ("fenerf_siren_density", "fenerf_siren_density_rays", "fenerf_render_density_workspace_bytes", "fenerf_render_density")


def test_lib_declares_the_entries_with_the_headers_argument_counts():
    hdr = open(os.path.join(ROOT, "include", "fenerf.h")).read()
    for name in ENTRIES:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\(([^;]*?)\);", hdr, re.S)
        assert m, name
        n_args = len([a for a in m.group(2).split(",") if a.strip()])
        res, args = _lib._SIGS[name]
        assert name in _lib.EXPORTS and len(args) == n_args, (name, len(args), n_args)
        assert res is (_lib._sz if m.group(1) == "size_t" else _lib._i)
    # the integer and size arguments sit where the header has them
    assert _lib._SIGS["fenerf_siren_density"][1][2] is _lib._i64 and _lib._SIGS["fenerf_siren_density"][1][6] is _lib._i
    assert _lib._SIGS["fenerf_siren_density_rays"][1][9] is _lib._i
    assert _lib._SIGS["fenerf_render_density"][1][14] is _lib._i and _lib._SIGS["fenerf_render_density"][1][20] is _lib._sz
    assert "FENERF_ABI_VERSION 2 " in hdr          # added entries change no struct and no signature


class StubModel:
    """what callers ask of a NativeModel; rows are a pure function of the point index"""

    def __init__(self, density, n_lab=18):
        self.density, self.n_lab, self.calls = density, n_lab, []

    def supports_density(self):
        return self.density

    def n_labels(self):
        return self.n_lab

    def _rows(self, P):
        g = torch.Generator().manual_seed(1)
        return torch.randn((1, P, self.n_lab + 4), generator=g)

    def siren_forward(self, points, ray_dirs, fg, pg, fa, pa):
        assert ray_dirs is None
        self.calls.append("forward")
        return self._rows(points.shape[1])

    def siren_density(self, points, fg, pg, labels=True, out=None):
        assert self.density, "the density query of a model that does not serve it"
        self.calls.append("density-labels" if labels else "density-sigma")
        rows = self._rows(points.shape[1])
        return torch.cat([rows[..., :self.n_lab], rows[..., -1:]], -1) if labels and self.n_lab else rows[..., -1].contiguous()


@pytest.mark.parametrize("n_lab", [18, 0])
def test_lattice_route_choice_and_fallback(n_lab):
    pts = torch.zeros((1, 50, 3))
    film = (None,) * 4
    dens, full = StubModel(True, n_lab), StubModel(False, n_lab)
    s1, l1 = callers._lattice_sigma(dens, pts, *film)
    s2, l2 = callers._lattice_sigma(full, pts, *film)
    assert dens.calls == ["density-sigma"] and full.calls == ["forward"] and l1 is None and l2 is None
    assert tuple(s1.shape) == (1, 50) and torch.equal(s1, s2)
    s1, l1 = callers._lattice_sigma(dens, pts, *film, want_labels=True)
    s2, l2 = callers._lattice_sigma(full, pts, *film, want_labels=True)
    assert dens.calls[-1] == ("density-labels" if n_lab else "density-sigma") and full.calls[-1] == "forward"
    assert torch.equal(s1, s2) and torch.equal(l1, l2) and l1.dtype == torch.uint8 and tuple(l1.shape) == (1, 50)
    if n_lab:
        assert torch.equal(l1[0].long(), torch.argmax(full._rows(50)[0, :, :n_lab], dim=-1))
    else:
        assert not bool(l1.any())


def test_argmax_label_takes_the_first_maximum():
    class Ties(StubModel):
        def _rows(self, P):
            rows = torch.zeros((1, P, 22))
            rows[0, :, 5] = 2.0
            rows[0, :, 9] = 2.0
            return rows
    _, lab = callers._lattice_sigma(Ties(True), torch.zeros((1, 4, 3)), None, None, None, None, want_labels=True)
    _, lab2 = callers._lattice_sigma(Ties(False), torch.zeros((1, 4, 3)), None, None, None, None, want_labels=True)
    assert lab.tolist() == [[5, 5, 5, 5]] and lab2.tolist() == [[5, 5, 5, 5]]


def test_render_multiview_cli_option_reaches_the_caller(monkeypatch, tmp_path):
    import render_multiview as tool
    opt = tool.build_parser().parse_args(["gen.pth"])
    assert opt.labels_only is False
    opt = tool.build_parser().parse_args(["gen.pth", "--labels_only", "--image_size", "8"])
    assert opt.labels_only is True
    seen = {}

    def fake_render_multiview(generator, curriculum, seed, device, **kw):
        seen.update(kw, seed=seed)
        assert kw.get("labels_only") is True
        return torch.zeros((5, 3, 8, 8)), torch.zeros((5, 8, 8))

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(callers, "load_generator", lambda *a, **k: object())
    monkeypatch.setattr(callers, "render_multiview", fake_render_multiview)
    tool.main(["gen.pth", "--labels_only", "--image_size", "8", "--seeds", "4", "--output_dir", str(tmp_path)])
    assert seen["labels_only"] is True and seen["seed"] == 4 and seen["image_size"] == 8
    assert sorted(os.listdir(tmp_path)) == ["grid_4_SEG.png"]          # the semantic row alone, under its usual name
    with pytest.raises(SystemExit):
        tool.main(["gen.pth", "--labels_only", "--geometry", "--output_dir", str(tmp_path)])
    with pytest.raises(SystemExit):
        tool.main(["gen.pth", "--labels_only", "--baked", "9", "--output_dir", str(tmp_path)])


def test_render_multiview_refuses_labels_only_with_other_routes():
    with pytest.raises(ValueError):
        callers.render_multiview(None, {0: dict(num_steps=3), "h_mean": 0.0}, 0, "cpu", labels_only=True, baked=9)
    with pytest.raises(ValueError):
        callers.render_multiview(None, {0: dict(num_steps=3), "h_mean": 0.0}, 0, "cpu", labels_only=True, geometry=True)


def test_extract_shapes_cli_option_reaches_the_caller(monkeypatch, tmp_path):
    import extract_shapes as tool
    from fenerf_amd import imageio_lite
    assert tool.build_parser().parse_args(["gen.pth"]).labels is False
    assert tool.build_parser().parse_args(["gen.pth", "--labels"]).labels is True
    seen = []
    vol = np.arange(27, dtype=np.float32).reshape(3, 3, 3)
    lab = (np.arange(27) % 18).astype(np.uint8).reshape(3, 3, 3)

    def fake_sample_generator(generator, z, **kw):
        seen.append(kw)
        return (vol, lab) if kw.get("return_labels") else vol

    class Gen:
        z_geo_dim = z_app_dim = 8

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch, "randn", lambda *a, **k: torch.zeros(a[:2]))
    monkeypatch.setattr(callers, "load_generator", lambda *a, **k: Gen())
    monkeypatch.setattr(callers, "sample_generator", fake_sample_generator)
    out = tmp_path / "with"
    tool.main(["gen.pth", "--labels", "--seeds", "3", "--voxel_resolution", "3", "--output_dir", str(out)])
    assert seen[-1]["return_labels"] is True and seen[-1]["voxel_resolution"] == 3
    assert sorted(os.listdir(out)) == ["3.mrc", "3_labels.npy"]
    assert np.array_equal(np.load(out / "3_labels.npy"), lab) and np.array_equal(imageio_lite.read_mrc(str(out / "3.mrc"))[0], vol)
    out = tmp_path / "without"
    tool.main(["gen.pth", "--seeds", "3", "--voxel_resolution", "3", "--output_dir", str(out)])
    assert "return_labels" not in seen[-1] and sorted(os.listdir(out)) == ["3.mrc"]         # defaults and file names as they were
