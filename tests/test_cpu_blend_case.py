"""tests/blend_case.py checked without a GPU: the restated chains reproduce the reference's recorded results; the gate is feasible for
the kernels' own order of operations (kernel_order) on every case tests/test_gpu_blend_edges.py runs, except its one big launch; the
gate rejects four structural mutants of that arithmetic, and the record of what the gate these kernels had before says to the same
mutants on the same cases ("blend" section, keeps the table).

A failing feasibility cell means the input or the gate is wrong, not a kernel.
"""
import functools
import os

import numpy as np
import pytest
import torch

import _util as U
import blend_case as bc


def _golden():
    g = np.load(os.path.join(U.GOLDEN, "blend_ref.npz"))
    return {k: (torch.from_numpy(g[k]) if g[k].ndim else g[k].item()) for k in g.files}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_chain_float32_reproduces_the_recorded_softmax_results(tag):
    g = _golden()
    k = lambda n: g[f"sm_{tag}_{n}"]  # noqa: E731
    zn, zf = (k(n) if isinstance(k(n), torch.Tensor) else float(k(n)) for n in ("znear", "zfar"))
    got = bc.chain(g["colors"], g["pix_to_face"], g["dists"], g["zbuf"], k("sigma"), k("gamma"), k("bg").tolist(), zn, zf,
                   torch.float32, k("grad_out"))
    assert torch.allclose(got["out"], k("out"), atol=1e-5, rtol=1e-5)
    for name in ("grad_colors", "grad_dists", "grad_zbuf"):
        ref = k(name)
        assert torch.allclose(got[name], ref, atol=1e-4 * max(1.0, ref.abs().max().item()), rtol=1e-3), name


def test_sigmoid_chain_float32_reproduces_the_recorded_results():
    g = _golden()
    got = bc.sigmoid_chain(g["pix_to_face"], g["dists"], g["sigma"], torch.float32, g["sig_grad_alphas"])
    assert torch.allclose(got["out"], g["sig_alphas"], atol=1e-6, rtol=0)
    ref = g["sig_grad_dists"]
    assert torch.allclose(got["grad_dists"], ref, atol=1e-6 * ref.abs().max().item(), rtol=1e-5)


@functools.lru_cache(maxsize=None)
def _case(K, pattern, gamma, default_params=False):
    """inputs and both chains of one case of the GPU file, computed once (mutants share them)"""
    N, H, W = bc.SHAPE
    gen = torch.Generator().manual_seed(bc.SEED + 10 * K + bc.PATTERNS.index(pattern))
    if default_params:
        sigma, zn, zf, bg = 1e-4, 1.0, 100.0, (1.0, 1.0, 1.0)
    else:
        sigma, zn, zf, bg = bc.SIGMA, bc.ZNEAR, bc.ZFAR, bc.BG
    x = bc.inputs(gen, N, H, W, K, sigma, pattern, zfar=zf)
    grad_out = torch.randn(N, H, W, 4, generator=gen)
    args = (x["colors"], x["pix_to_face"], x["dists"], x["zbuf"], sigma, gamma, bg, zn, zf)
    return x, grad_out, args, bc.chain(*args, torch.float32, grad_out), bc.chain(*args, torch.float64, grad_out)


@pytest.mark.parametrize("pattern", bc.PATTERNS)
@pytest.mark.parametrize("K", bc.CAPACITIES)
def test_kernel_order_is_inside_the_gate(K, pattern):
    for gamma in bc.GAMMAS:
        x, grad_out, args, c32, c64 = _case(K, pattern, gamma)
        present = {bc.CLASSES[i] for i in x["classes"].unique().tolist()}
        assert present == set(bc.CLASSES) - ({"tie"} if K < 2 else set())
        for c in c64.values():
            assert bool(torch.isfinite(c).all())
        got = bc.kernel_order(*args, grad_out)
        assert bc.gate(got, c32, c64, x["classes"], label=f"K={K} {pattern} gamma={gamma}") == []


@pytest.mark.parametrize("K", [2, 8, 33])
def test_kernel_order_is_inside_the_gate_at_default_parameters(K):
    x, grad_out, args, c32, c64 = _case(K, "prefix", 1e-4, True)
    got = bc.kernel_order(*args, grad_out)
    assert bc.gate(got, c32, c64, x["classes"], label=f"K={K} BlendParams()") == []


MUTANT_CASES = [(K, pattern, gamma) for K in (2, 5, 8, 33) for pattern in ("prefix", "full") for gamma in bc.GAMMAS]


def _verdicts(mutant):
    """[(case, rejected by the gate on some class, accepted by the old gate)]"""
    rows = []
    for K, pattern, gamma in MUTANT_CASES:
        x, grad_out, args, c32, c64 = _case(K, pattern, gamma)
        got = bc.kernel_order(*args, grad_out, mutant=mutant)
        missed = bc.gate(got, c32, c64, x["classes"], show=lambda line: None)
        rows.append(((K, pattern, gamma), missed, bc.old_gate(got, c64)))
    return rows


@pytest.mark.parametrize("mutant", bc.MUTANTS)
def test_the_gate_rejects_the_mutant(mutant):
    rows = _verdicts(mutant)
    cells = [(case, q, cname) for case, missed, _ in rows for q, cname, _, _ in missed]
    print(mutant, "rejected in", len(cells), "(case, quantity, class) cells, first:", cells[:3])
    assert cells


def test_old_gate_record():
    """What the former gate says to the same mutants on the same cases: printed, and kept in DESIGN.md."""
    print("mutant | cases the new gate rejects | cases the old gate accepts | cases only the new gate rejects")
    for mutant in bc.MUTANTS:
        rows = _verdicts(mutant)
        new = sum(bool(missed) for _, missed, _ in rows)
        old = sum(accepted for _, _, accepted in rows)
        only = [case for case, missed, accepted in rows if missed and accepted]
        print(f"{mutant} | {new} of {len(rows)} | {old} of {len(rows)} | {len(only)}: {only}")
    # the unmutated arithmetic passes both
    for K, pattern, gamma in MUTANT_CASES:
        x, grad_out, args, c32, c64 = _case(K, pattern, gamma)
        got = bc.kernel_order(*args, grad_out)
        assert bc.old_gate(got, c64) and bc.gate(got, c32, c64, x["classes"], show=lambda line: None) == []
