"""The refusals of the differentiable C-ABI entries that share one preamble (model, tape format, differentiable, B / P, first pointer
check) and one gradient-buffer check (fenerf_api.cpp diff_preamble / check_grads): one fault at a time, status code and the whole
fenerf_last_error() text.  Every call here is refused before anything is launched; the one device buffer all pointers name is never
touched."""
import ctypes as C

import pytest
import torch

from test_gpu_parity import DEV
from fenerf_amd import _lib, native, procedural as proc

pytestmark = pytest.mark.gpu

INV, UNS = _lib.E_INVALID, _lib.E_UNSUPPORTED
NOT_DIFF = (UNS, "model was not created with differentiable != 0")
BAD_B = (INV, "B must be > 0 and P >= 0")
BAD_P = (INV, "differentiable path: points per image must be a multiple of 32")
NULLP = (INV, "NULL pointer")
BAD_FMT = (INV, "unknown tape format")
FILM_NULL = (INV, "grads: film pointer is NULL")
ALL_OR_NONE = (INV, "grads: give every weight / bias buffer or none (FiLM gradients only)")
ALL_REQUIRED = (INV, "grads: every weight / bias buffer is required")
BAD_BRN = (INV, "need B, R > 0 and 3 <= num_steps <= 512 (hierarchical render; FENERF_MAX_RAY_SAMPLES / 2)")
SAVE_SMALL = (INV, "save buffer too small (see fenerf_render_save_bytes)")
WS_SMALL = (INV, "workspace too small (see fenerf_render_backward_workspace_bytes / _split_workspace_bytes)")
WS_SMALL_RAYS = (INV, "workspace too small (see fenerf_render_backward_rays_workspace_bytes)")

KINDS = [(grid, prec) for grid in (False, True) for prec in ("f32", "f16x3")]


@pytest.fixture(scope="module")
def world():
    """{(grid, precision, differentiable): NativeModel} at H = 32 (8^3 grid), and the buffer every pointer argument names"""
    models = {}
    for grid in (False, True):
        spec = proc.model_spec("texture", hidden_dim=32, grid_size=8) if grid else proc.model_spec("baseline", hidden_dim=32)
        sd = proc.make_state_dict(spec, seed=0, with_mapping=False)
        for prec in ("f32", "f16x3"):
            for diff in (False, True):
                models[grid, prec, diff] = native.NativeModel(sd, spec, DEV, prec, differentiable=diff)
    buf = torch.zeros(8 << 20, dtype=torch.uint8, device=DEV)
    return models, C.c_void_p(buf.data_ptr()), buf


def _grads(nat, p, drop=None):
    """a FenerfSirenGrads with every buffer the model has set to `p`, but `drop` (a field, or (field, index))"""
    g = _lib.FenerfSirenGrads()
    for i in range(nat.spec["n_geo"]):
        g.geo_w[i], g.geo_b[i] = p.value, p.value
    for i in range(nat.spec["n_color"]):
        g.color_w[i], g.color_b[i] = p.value, p.value
    for k in ("head_w", "head_b", "rgb_w", "rgb_b", "d_freq_geo", "d_phase_geo", "d_freq_app", "d_phase_app"):
        setattr(g, k, p.value)
    if isinstance(drop, tuple):
        getattr(g, drop[0])[drop[1]] = None
    elif drop:
        setattr(g, drop, None)
    return g


# entry -> its arguments behind (model, B, P), in order; "p" = the device buffer, "g" = a complete FenerfSirenGrads, "fmt" = FENERF_TAPE_F32
FILM = ["fg", "pg", "fa", "pa"]
ENTRIES = {
    "fenerf_siren_forward_save_fmt": ["points", "ray_dirs"] + FILM + ["out", "tape", "tape_e", "film_ws", "fmt", "stream"],
    "fenerf_siren_backward_fmt": FILM + ["out", "d_out", "tape", "fmt", "d_t", "d_e", "film_ws", "stream"],
    "fenerf_siren_backward_film": FILM + ["out", "d_out", "tape", "film_sums", "film_ws", "stream"],
    "fenerf_siren_film_grads": FILM + ["film_sums", "g", "workspace", "film_ws", "stream"],
    "fenerf_siren_backward_grid_fmt": FILM + ["out", "d_out", "tape", "fmt", "points", "d_t", "d_grid_cl", "scratch_d_e", "film_ws", "stream"],
    "fenerf_siren_param_grads_fmt": ["points", "ray_dirs"] + FILM + ["out", "d_out", "tape", "fmt", "tape_e", "d_t", "g", "weights", "workspace", "film_ws",
                                                                     "stream"],
    "fenerf_siren_input_grads": ["points"] + FILM + ["d_t", "w_geo0", "w_color0", "ld", "d_points", "d_dirs", "film_ws", "stream"],
    "fenerf_siren_forward_save_pointwise": ["points", "ray_dirs"] + FILM + ["out", "tape", "film_ws", "stream"],
    "fenerf_siren_backward_pointwise": FILM + ["out", "d_out", "tape", "d_t", "film_ws", "prepared", "stream"],
    "fenerf_siren_param_grads_pointwise": ["points", "ray_dirs"] + FILM + ["out", "d_out", "tape", "d_t", "g", "workspace", "film_ws", "prepared", "stream"],
}
# entry -> which (grid, precision) models it serves
SERVES = {
    "fenerf_siren_backward_film": [k for k in KINDS if k[1] == "f16x3"],
    "fenerf_siren_film_grads": [k for k in KINDS if k[1] == "f16x3"],
    "fenerf_siren_backward_grid_fmt": [k for k in KINDS if k[0]],
    "fenerf_siren_forward_save_pointwise": [(False, "f32")],
    "fenerf_siren_backward_pointwise": [(False, "f32")],
    "fenerf_siren_param_grads_pointwise": [(False, "f32")],
}
# entry -> [(argument to replace, value, expected)] beside the faults every entry is given
OWN = {
    "fenerf_siren_forward_save_fmt": [("out", None, (INV, "points / out / tape is NULL")), ("fmt", 7, BAD_FMT), ("film_ws", None, (INV, "film workspace is NULL"))],
    "fenerf_siren_backward_fmt": [("d_t", None, NULLP), ("fmt", 7, BAD_FMT), ("fg", None, (INV, "freq_geo / phase_geo is NULL")),
                                  ("fa", None, (INV, "freq_app / phase_app is NULL"))],
    "fenerf_siren_backward_film": [("film_sums", None, NULLP)],
    "fenerf_siren_film_grads": [("workspace", None, NULLP), ("g", "d_phase_app", FILM_NULL)],
    "fenerf_siren_backward_grid_fmt": [("out", None, NULLP), ("fmt", 7, BAD_FMT), ("points", None, (INV, "points / d_grid_cl is NULL"))],
    "fenerf_siren_param_grads_fmt": [("d_t", None, NULLP), ("fmt", 7, BAD_FMT), ("g", "d_freq_geo", FILM_NULL), ("g", ("geo_b", 1), ALL_OR_NONE),
                                     ("g", "rgb_w", ALL_OR_NONE)],
    "fenerf_siren_input_grads": [("w_geo0", None, (INV, "d_t / w_geo0 / w_color0 is NULL"))],
    # (the per-point entries prepare the FiLM blocks before they look at their other pointers: film_ws_prepared = 1 here, so nothing runs)
    "fenerf_siren_forward_save_pointwise": [("fg", None, (INV, "film parameter / workspace pointer is NULL"))],
    "fenerf_siren_backward_pointwise": [("d_t", None, NULLP), ("film_ws", None, (INV, "film parameter / workspace pointer is NULL"))],
    "fenerf_siren_param_grads_pointwise": [("workspace", None, NULLP), ("g", "d_freq_app", FILM_NULL), ("g", ("color_w", 0), ALL_REQUIRED),
                                           ("g", "head_b", ALL_REQUIRED)],
}
# pointers that only a model with a feature grid needs
GRID_ONLY = {
    "fenerf_siren_forward_save_fmt": [("tape_e", (INV, "points / out / tape is NULL"))],
    "fenerf_siren_backward_fmt": [("d_e", NULLP)],
    "fenerf_siren_param_grads_fmt": [("tape_e", NULLP)],
}


def _refused(l, rc, want, what):
    assert (rc, l.fenerf_last_error().decode()) == want, what


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_point_entries_refuse_one_fault_at_a_time(world, entry):
    models, p, _ = world
    l = _lib.lib()
    fn = getattr(l, entry)
    for grid, prec in SERVES.get(entry, KINDS):
        nat = models[grid, prec, True]

        def call(model=nat, B=1, P=32, **over):
            vals = dict(fmt=_lib.TAPE_F32, ld=3 + 32 + 32, prepared=1, stream=None, weights=None)
            args = []
            for name in ENTRIES[entry]:
                v = over[name] if name in over else vals.get(name, p)
                if name == "g":
                    v = _grads(model, p, drop=over.get("g"))
                    v = C.byref(v)
                args.append(v)
            return fn(model._h, B, P, *args)

        _refused(l, call(model=models[grid, prec, False]), NOT_DIFF, (entry, grid, prec, "not differentiable"))
        _refused(l, call(B=0), BAD_B, (entry, grid, prec, "B = 0"))
        _refused(l, call(P=48), BAD_P, (entry, grid, prec, "P = 48"))
        for name, value, want in OWN[entry]:
            _refused(l, call(**{name: value}), want, (entry, grid, prec, name, value))
        for name, want in GRID_ONLY.get(entry, []) if grid else []:
            _refused(l, call(**{name: None}), want, (entry, grid, prec, name))


@pytest.mark.parametrize("grid,prec", KINDS)
def test_render_backward_refuses_one_fault_at_a_time(world, grid, prec):
    """fenerf_render_backward, _rays and _stage: the same faults, and a save buffer / workspace one byte short of what the size entries ask for"""
    models, p, _ = world
    l = _lib.lib()
    nat = models[grid, prec, True]
    B, R, N = 1, 4, 4
    opts = _lib.composite_opts("relu", 0.0)
    save_bytes = l.fenerf_render_save_bytes(nat._h, B, R, N, 0, 0)
    ws_bytes = l.fenerf_render_backward_workspace_bytes(nat._h, B, R, N, 0, 0, 0)
    rays_bytes = l.fenerf_render_backward_rays_workspace_bytes(nat._h, B, R, N, 0, 0, 0, 0)
    split_bytes = l.fenerf_render_backward_split_workspace_bytes(nat._h, B, R, N, 0, 1)
    assert 0 < save_bytes and 0 < ws_bytes < rays_bytes and ws_bytes <= split_bytes

    def call(model=nat, B=B, save=p, save_bytes=save_bytes, fmt=0, drop=None, ws_bytes=ws_bytes, d_grid=p, entry="plain"):
        g = _grads(model, p, drop)
        head = (B, R, N, 0, save, save_bytes, fmt, p, None, C.byref(opts), p, C.byref(g), d_grid, None, 0)
        if entry == "plain":
            return l.fenerf_render_backward(model._h, *head, 0, p, ws_bytes, None)
        if entry == "rays":
            return l.fenerf_render_backward_rays(model._h, *head, 0, p, ws_bytes, p, p, 3 + 32 + 32, p, p, None)
        return l.fenerf_render_backward_stage(model._h, 1, 1, *head, p, ws_bytes, None)

    for entry, full, small in (("plain", ws_bytes, WS_SMALL), ("rays", rays_bytes, WS_SMALL_RAYS), ("stage", split_bytes, WS_SMALL)):
        what = (entry, grid, prec)
        _refused(l, call(model=models[grid, prec, False], ws_bytes=full, entry=entry), NOT_DIFF, what)
        _refused(l, call(B=0, ws_bytes=full, entry=entry), BAD_BRN, what)
        _refused(l, call(save=None, ws_bytes=full, entry=entry), NULLP, what)
        _refused(l, call(fmt=7, ws_bytes=full, entry=entry), BAD_FMT, what)
        _refused(l, call(drop="d_phase_geo", ws_bytes=full, entry=entry), FILM_NULL, what)
        _refused(l, call(drop=("geo_w", 2), ws_bytes=full, entry=entry), ALL_OR_NONE, what)
        _refused(l, call(save_bytes=save_bytes - 1, ws_bytes=full, entry=entry), SAVE_SMALL, what)
        _refused(l, call(ws_bytes=full - 1, entry=entry), small, what)
        if grid:
            _refused(l, call(d_grid=None, ws_bytes=full, entry=entry), (INV, "d_grid_ncdhw is NULL"), what)
