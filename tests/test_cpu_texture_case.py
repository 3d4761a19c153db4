"""tests/texture_case.py without a GPU: its float32 chain reproduces the reference's recorded results, the oracle's restatement
(kernel_order) and the explicit one (restated) pass the gate on every case of tests/test_gpu_texture_edges.py, every mutant fails it, the
mirrored table constants are those of csrc/texture.hip, and csrc/atlas_cell.h agrees with torch's own indexing on its edges."""
import ctypes
import os
import re

import pytest
import torch

import _util as U
import texture_case as tc
from test_cpu_texuv_multi_oracle import load_multi
from test_cpu_texuv_oracle import CASES, load, uv_vertex_grads

CSRC = os.path.join(U.ROOT, "pytorch3d_amd", "csrc")
MODE_OF = {tag: (kw["align_corners"], kw["padding_mode"], kw["sampling_mode"]) for tag, kw in CASES.items()}


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-3, atol=2e-5 * max(1.0, b.abs().max().item()))


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("tag", list(CASES))
def test_float32_chain_reproduces_the_recorded_reference(tag, multi):
    g, fu, idx = load_multi() if multi else load()
    x = {"pix_to_face": g["pix_to_face"], "bary": g["bary"], "face_uvs": fu, "maps": g["maps"], "grad_texels": g[f"{tag}_grad_texels"]}
    if multi:
        x["maps_ids"] = g["maps_ids"]
    r = tc.chain(x, MODE_OF[tag], torch.float32)
    ref = g[f"{tag}_texels"]
    assert torch.allclose(r["texels"], ref, atol=1e-5, rtol=1e-5), (r["texels"] - ref).abs().max()
    assert _close(r["grad_maps"], g[f"{tag}_grad_maps"])
    assert _close(r["grad_bary"], g[f"{tag}_grad_bary"])
    assert _close(uv_vertex_grads(r["grad_face_uvs"], idx, g["verts_uvs"].shape[0]), g[f"{tag}_grad_verts_uvs"])


def _gate_case(kind, *args, how=tc.kernel_order):
    x, c32, c64 = tc.case(kind, *args)
    mode = args[-1]
    label = f"{kind} {' '.join(str(a) for a in args[:-1])} {tc.mode_id(mode)}"
    assert tc.gate(how(x, mode), c32, c64, x, mode, label=label) == []
    return x


@pytest.mark.parametrize("mode", tc.MODES, ids=tc.mode_id)
@pytest.mark.parametrize("C", tc.CHANNELS)
def test_kernel_order_passes_the_gate_single_map(C, mode):
    x = _gate_case("main", C, mode)
    assert tc.flushes_mid_span(x, mode), tc.reach(x, mode)
    assert {tc.CLASSES[i] for i in x["classes"].unique().tolist()} == set(tc.CLASSES)


@pytest.mark.parametrize("mode", tc.MODES, ids=tc.mode_id)
def test_kernel_order_passes_the_gate_small_lattice_and_multi_maps(mode):
    for size in tc.SMALL_MAPS:
        _gate_case("small", size, mode)
    for size in tc.LATTICE_MAPS:
        _gate_case("lattice", size, mode)
    for M, C in tc.MULTI:
        _gate_case("multi", M, C, mode)


@pytest.mark.parametrize("mode", tc.MODES, ids=tc.mode_id)
def test_explicit_restatement_passes_the_gate(mode):
    _gate_case("main", 3, mode, how=tc.restated)
    _gate_case("lattice", tc.LATTICE_MAPS[0], mode, how=tc.restated)
    _gate_case("multi", 3, 3, mode, how=tc.restated)


MUTANT_CASES = {"map_of_image_0": ("main", 3, (True, "border", "bilinear")),
                "background_map_grad_dropped": ("main", 3, (True, "border", "bilinear")),
                "lost_step": ("main", 3, (True, "border", "bilinear")),
                "border_keeps_multiplier": ("main", 3, (False, "border", "bilinear")),
                "half_away_from_zero": ("lattice", (8, 16), (False, "zeros", "nearest")),
                "iz_rounded": ("multi", 3, 3, (False, "zeros", "bilinear"))}


@pytest.mark.parametrize("mutant", tc.MUTANTS)
def test_every_mutant_fails_the_gate(mutant):
    kind, *args = MUTANT_CASES[mutant]
    mode = args[-1]
    x, c32, c64 = tc.case(kind, *args)
    got = tc.restated(x, mode, mutant)
    failures = tc.gate(got, c32, c64, x, mode, show=lambda s: None)
    old = tc.old_gate(got, tc.kernel_order(x, mode))
    print(f"MUTANT {mutant:28s} {kind:8s} {tc.mode_id(mode):24s} new gate rejects {sorted({q for q, *_ in failures})}; "
          f"the former gate {'accepts' if old else 'rejects'}")
    assert failures
    x0 = x["pix_to_face"].reshape(x["pix_to_face"].shape[0], -1)[tc.LOST_STEP[0], tc.LOST_STEP[1] * 64:][:64]
    assert mutant != "lost_step" or bool((x0 >= 0).all())


def test_mirrored_constants_are_those_of_the_kernel():
    src = open(os.path.join(CSRC, "texture.hip")).read()
    assert int(re.search(r"using UvTable = WaveTable<6, (\d+), kRows>;", src).group(1)) == tc.UV_SLOTS
    assert int(re.search(r"using TexelTable = WaveTable<4, (\d+), kChunk>;", src).group(1)) == tc.TEXEL_SLOTS
    assert int(re.search(r"int64_t waves = ceil_div\(HWK, (\d+)\);", src).group(1)) == tc.SPAN_SAMPLES
    assert re.search(r"if \(waves > 4 \* 16384\) waves = 4 \* 16384;", src) and tc.MAX_WAVES == 4 * 16384
    assert "const int64_t bx = ceil_div(waves, 4);" in src
    assert "const int64_t span = ceil_div(ceil_div(HWK, bx * 4), 64) * 64;" in src
    table = open(os.path.join(CSRC, "wave_table.h")).read()
    assert int(re.search(r"kFlushAt = SPILL \? SLOTS \* 3 / 4 : SLOTS - (\d+);", table).group(1)) == tc.RESERVE
    assert tc.span_of(3072) == 768 and tc.span_of(4097) == 1088 and tc.span_of(256) == 64 and tc.span_of(4096 * 8 + 1) == 2752


@pytest.mark.parametrize("R", [1, 2, 7])
def test_atlas_cell_edges_against_torch_indexing(R):
    """csrc/atlas_cell.h (the host build) on barycentrics 0 and 1, the diagonal b0 + b1 = 1, (R-1)/R, negatives that wrap, values below
    -1, NaN and +-inf, against the indexing expression of TexturesAtlas.sample_textures evaluated by torch, sample by sample: the
    cell it reads, or -1 where torch raises an IndexError."""
    nan, inf = float("nan"), float("inf")
    vals = [0.0, 1.0, 0.5, (R - 1) / R, 1.0 / R, 1.0 - 1.0 / (2 * R), -0.0, -1e-7, -0.25, -0.5, -1.0 / R, -1.0, -1.0 - 1e-6, -1.5, -3.0, 2.0,
            1e19, -1e19, nan, inf, -inf]
    pairs = [(a, b) for a in vals for b in vals] + [(k / (4.0 * R), 1.0 - k / (4.0 * R)) for k in range(4 * R + 1)]
    b = torch.tensor(pairs, dtype=torch.float32)
    bary = torch.cat([b, (1.0 - b.sum(-1, keepdim=True))], -1).contiguous()
    n = bary.shape[0]
    cells = torch.empty(n, dtype=torch.int64)
    U.hostgeom().hg_atlas_cells(U.p(bary), ctypes.c_int64(n), R, U.p(cells))
    marker = torch.arange(R * R).view(1, R, R)
    w_y, w_x = tc.atlas_cells(bary, R)
    want = []
    for i in range(n):
        try:
            want.append(int(marker[torch.zeros(1, dtype=torch.int64), w_y[i:i + 1], w_x[i:i + 1]]))
        except IndexError:
            want.append(-1)
    want = torch.tensor(want)
    differ = (cells != want).nonzero().flatten().tolist()
    assert not differ, [(pairs[i], int(cells[i]), int(want[i])) for i in differ[:8]]
    assert int((want >= 0).sum()) > n // 8 and int((want < 0).sum()) > 0
