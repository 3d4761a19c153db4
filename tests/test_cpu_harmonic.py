"""HarmonicEmbedding and the stratified depths without a GPU: every case of tests/harmonic_case.py through the torch formulations and the
same gates as the kernels, six wrong variants of the formulation refused by those gates (and cos(t) judged by gate 1), the
declarations and constants of the three new entries, and the path predicates by shape arithmetic."""
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import harmonic_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _C, _lib  # noqa: E402

H = importlib.import_module("pytorch3d_amd.harmonic_embedding")  # (the package exports a function of the module's name)
RS = importlib.import_module("pytorch3d_amd.raysampling")
CASES = C.cases()
ENTRIES = ("p3di_harmonic_embedding_forward", "p3di_harmonic_embedding_backward", "p3di_stratified_depths")
MACROS = ("HARMONIC_FWD_ROWS", "HARMONIC_BWD_ROWS", "HARMONIC_BWD_LDS_FLOATS", "HARMONIC_MAX_WIDTH", "HARMONIC_MAX_GROUPS")


def restated(x, f, cov, append, wrong=None, omega=1.0):
    """The contract of csrc/implicit_abi.h written out index by index in torch, with the wrong variants the gates must refuse."""
    if wrong == "omega":
        f = f / omega  # omega_0 dropped
    t = x[..., :, None] * f  # (..., dim, n)
    c = torch.tensor([0.0, float(C.HALF_PI32)], dtype=x.dtype)
    if wrong == "swap":
        c = c.flip(0)
    if wrong == "cos":
        blocks = torch.stack([t.sin(), t.cos()], dim=-3)
    else:
        blocks = (t[..., None, :, :] + c[:, None, None]).sin()  # (..., 2, dim, n)
    if cov is not None:
        power = f if wrong == "f1" else f * f
        blocks = blocks * torch.exp((0.5 if wrong == "plus" else -0.5) * (cov[..., :, None] * power))[..., None, :, :]
    if wrong == "transposed":
        blocks = blocks.transpose(-1, -2)
    flat = blocks.reshape(*x.shape[:-1], 2 * x.shape[-1] * f.shape[0])
    if not append:
        return flat
    return torch.cat([x, flat] if wrong == "front" else [flat, x], dim=-1)


def test_fixture_holds_every_case_and_the_cases_hold_every_size():
    fix = C.fixture()
    for case in CASES:
        assert fix[C.key(case.id, "out")].shape == case.lead + (C.width(case),), case.id
        assert fix[C.key(case.id, "grad_x")].shape == case.lead + (case.dim,), case.id
        assert (C.key(case.id, "grad_cov") in fix) == (case.cov is not None), case.id
    rows = {int(np.prod(c.lead, dtype=np.int64)) for c in CASES}
    assert {1, 2, 63, 64, 65, 257} <= rows
    # one row below, at and above both tiles, by the header's constants: 64 rows forward, 64 backward at narrow rows ...
    assert _lib.HARMONIC_FWD_ROWS == 64 and C.backward_tile_rows(3, _lib) == 64 == _C.harmonic_embedding_backward_tile_rows(3)
    assert C.width(C.case_by_id("rows64")) == 3 and C.width(C.case_by_id("small-d3-n6-r65-a1")) == 39
    # ... and the LDS-limited tile of the widest case: 30 rows of 268 floats at stride 269, with 31 rows in the case
    wide = next(c for c in CASES if C.width(c) == 268 and c.lead == (31,))
    assert C.backward_tile_rows(268, _lib) == 30 == _lib.HARMONIC_BWD_LDS_FLOATS // 269
    assert wide.lead[0] == C.backward_tile_rows(268, _lib) + 1
    assert {c.dim for c in CASES} >= {1, 2, 3, 4} and {c.n for c in CASES} >= {1, 4, 6, 10, 16, 33}
    assert {c.append for c in CASES} == {True, False} and {c.logspace for c in CASES} == {True, False}
    assert {round(c.omega, 4) for c in CASES} == {1.0, 0.1, round(math.pi, 4)} and any(c.freqs == "hand" for c in CASES)
    assert {c.lead for c in CASES} >= {(), (5,), (2, 3, 7)} and {c.layout for c in CASES} == {"contiguous", "transposed", "slice"}
    pools = {}
    for c in CASES:
        if not c.special:
            pools[C.pool(c)] = pools.get(C.pool(c), 0) + 1
    assert min(pools.values()) >= 6 and len(pools) == 9, pools
    for name in pools:
        assert float(fix[f"E_ref/{name}/out"]) > 0 and float(fix[f"E_ref/{name}/grad_x"]) > 0
    assert 1e-8 < float(fix["E_sin"]) < 1.2e-7 and 1e-8 < float(fix["E_exp"]) < 2.4e-7  # about an ulp of a value near 1
    sp = C.case_by_id("special")
    assert fix[C.key(sp.id, "nonfinite_out")].any() and not fix[C.key(sp.id, "nonfinite_out")][1].any()
    assert np.array_equal(fix[C.key(sp.id, "nonfinite_out")], ~np.isfinite(fix[C.key(sp.id, "out")]))


def test_torch_formulation_module_and_restatement_pass_the_gates():
    assert C.failures(CASES, H.harmonic_embedding_torch) == []
    assert C.failures(CASES, A.harmonic_embedding) == []  # CPU tensors: the chain
    assert C.failures(CASES, restated) == []


def test_every_needs_input_grad_combination_on_the_chain():
    for cid in ("cov-d3-n4", "small-d3-n10-r5-a1"):
        for need in ((True, False), (False, True), (False, False)):
            assert C.failures([C.case_by_id(cid)], A.harmonic_embedding, need=need) == []


def test_module_is_the_reference_s_and_equals_the_function():
    for case in (c for c in CASES if c.freqs == "module" and not c.special):
        module = A.HarmonicEmbedding(case.n, case.omega, case.logspace, case.append)
        x, cov, f, _ = C.inputs(case)
        assert torch.equal(module._frequencies, f) and module._zero_half_pi.dtype == torch.float32
        assert float(module._zero_half_pi[1]) == float(C.HALF_PI32) and float(module._zero_half_pi[0]) == 0.0
        assert torch.equal(module(x, diag_cov=cov), A.harmonic_embedding(x, f, cov, case.append)), case.id
        assert module.get_output_dim(case.dim) == C.width(case) == A.HarmonicEmbedding.get_output_dim_static(case.dim, case.n, case.append)
    module = A.HarmonicEmbedding()
    assert len(module._frequencies) == 6 and module.append_input and module.get_output_dim() == 39
    assert list(module.state_dict()) == []  # both buffers are non-persistent
    assert module.double()(torch.zeros(2, 3, dtype=torch.float64)).dtype == torch.float64
    assert module(torch.zeros(2, 3, dtype=torch.float64), some_keyword=1).shape == (2, 39)


def test_zero_rows_and_n_of_zero_give_the_right_shapes():
    f = torch.tensor([1.0, 2.0])
    assert A.harmonic_embedding(torch.zeros(0, 3), f).shape == (0, 15)
    assert A.harmonic_embedding(torch.zeros(4, 0, 3), f, append_input=False).shape == (4, 0, 12)
    assert A.harmonic_embedding(torch.zeros(0, 3), f, torch.zeros(0, 3)).shape == (0, 15)
    x = torch.rand(5, 3)
    assert torch.equal(A.harmonic_embedding(x, torch.zeros(0)), x) and A.HarmonicEmbedding(0)(x).shape == (5, 3)


WRONG = {"swap": "small-d3-n10-r5-a1", "transposed": "small-d3-n10-r5-a1", "omega": "small-omegapi", "front": "small-d3-n10-r5-a1",
         "plus": "cov-d3-n4", "f1": "cov-d3-n4"}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_variants_are_refused_by_the_gates(wrong):
    case = C.case_by_id(WRONG[wrong])

    def fn(x, f, cov, append):
        return restated(x, f, cov, append, wrong=wrong, omega=case.omega)

    assert C.failures([case], restated) == []
    bad = C.failures([case], fn)
    assert bad, wrong
    every = [c for c in CASES if not c.special and (c.cov if wrong in ("plus", "f1") else True) and (c.omega != 1.0 if wrong == "omega" else True)
             and (c.append if wrong == "front" else True) and (c.dim > 1 or c.n > 1)]
    if wrong == "transposed":
        every = [c for c in every if c.dim > 1 and c.n > 1]
    refused = [c.id for c in every if C.failures([c], lambda x, f, cov, append, c=c: restated(x, f, cov, append, wrong=wrong, omega=c.omega))]
    assert len(refused) == len(every), sorted(set(c.id for c in every) - set(refused))


def test_cos_of_t_in_place_of_sin_of_t_plus_half_pi_is_judged_by_gate_1():
    """cos(t) is not the contract.  Whether the gates accept it is decided by gate 1 alone: it is the better value of cos(x f), and
    further from the reference's sin(fl(t + pi/2)) the larger t is.  Printed: the ratio to gate 1 per pool; it is refused in every pool
    but those where fl(t + pi/2) loses nothing that matters."""
    fix = C.fixture()
    gate1 = C.GATE_FACTOR * float(fix["E_sin"])
    worst = {}
    for case in (c for c in CASES if not c.special and not c.cov):
        x, _, f, _ = C.inputs(case)
        out = restated(x, f, None, case.append, wrong="cos").double().numpy()
        err = C.argument_error(case, out)
        worst[C.pool(case)] = max(worst.get(C.pool(case), 0.0), err / gate1)
        refused = any("gate 1" in b for b in C.failures([case], lambda x, f, cov, append: restated(x, f, cov, append, wrong="cos")))
        assert refused == (err > gate1), case.id  # accepted only if it is within gate 1
    print({k: round(v, 2) for k, v in sorted(worst.items())})
    assert worst["large-log"] > 1 and worst["scene-log"] > 1 and worst["octaves-log"] > 1  # refused wherever the arguments are not tiny
    assert max(worst.values()) > 1000


def test_declarations_constants_and_exports():
    lib = _lib.load()
    header = open(_lib.EXTENSION_HEADER_PATH).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXTENSION_DECLARATIONS and name in _lib.EXTENSION_SYMBOLS
        assert name not in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    for name in MACROS:
        assert name in _lib.EXTENSION_CONSTANTS and getattr(_lib, name) == _lib.EXTENSION_CONSTANTS[name] > 0
    assert (_lib.HARMONIC_MAX_WIDTH | 1) <= _lib.HARMONIC_BWD_LDS_FLOATS < ((_lib.HARMONIC_MAX_WIDTH + 1) | 1)
    assert _lib.EXTENSION_DECLARATIONS["p3di_stratified_depths"][1][1] == "const int64_t[2]"
    from pytorch3d_amd import build

    assert "harmonic.hip" in build.SOURCES
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, exported, re.M), name
    assert {"harmonic_embedding", "HarmonicEmbedding", "harmonic_embedding_torch", "stratified_depths"} <= set(dir(A))
    assert "harmonic_embedding" in A.__doc__ and "stratified_depths" in A.__doc__


def test_c_abi_status_codes_without_a_launch():
    lib = _lib.load()
    one = torch.zeros(4)
    p = one.data_ptr()
    fwd, bwd, dep = lib.p3di_harmonic_embedding_forward, lib.p3di_harmonic_embedding_backward, lib.p3di_stratified_depths
    assert fwd(None, None, None, 0, 3, 10, 1, None, None) == _lib.OK  # no rows: no launch, no pointer read
    for rows, dim, n, append in ((-1, 3, 10, 1), (1, 0, 10, 1), (1, 3, 0, 1), (1, 3, 10, 2), (1, 1, _lib.HARMONIC_MAX_WIDTH // 2 + 1, 0),
                                 (2 ** 31 // 63 + 1, 3, 10, 1), (1, 2 ** 40, 2 ** 40, 1)):
        assert fwd(p, None, p, rows, dim, n, append, p, None) == _lib.ERR_INVALID_ARG, (rows, dim, n, append)
        assert bwd(p, None, p, p, rows, dim, n, append, p, None, None) == _lib.ERR_INVALID_ARG, (rows, dim, n, append)
    assert fwd(None, None, p, 1, 1, 1, 0, p, None) == _lib.ERR_INVALID_ARG and fwd(p, None, p, 1, 1, 1, 0, None, None) == _lib.ERR_INVALID_ARG
    assert bwd(p, None, p, p, 1, 1, 1, 0, None, p, None) == _lib.ERR_INVALID_ARG  # grad_cov without diag_cov
    assert bwd(p, None, p, p, 1, 1, 1, 0, None, None, None) == _lib.OK  # nothing asked for
    assert bwd(p, None, p, None, 1, 1, 1, 0, p, None, None) == _lib.ERR_INVALID_ARG
    two = (_lib.c_i64 * 2)(1, 1)
    assert dep(None, two, 0, 5, None, None, None) == _lib.OK and dep(None, two, 5, 0, None, None, None) == _lib.OK
    assert dep(p, two, -1, 1, p, p, None) == _lib.ERR_INVALID_ARG and dep(p, two, 2 ** 20, 2 ** 12, p, p, None) == _lib.ERR_INVALID_ARG
    assert dep(p, (_lib.c_i64 * 2)(-1, 1), 1, 1, p, p, None) == _lib.ERR_INVALID_ARG and dep(None, two, 1, 1, p, p, None) == _lib.ERR_INVALID_ARG


class _Fake:
    """A tensor's shape, dtype and device without its memory: kernel_path reads nothing else."""

    def __init__(self, shape, dtype=torch.float32, cuda=True, requires_grad=False):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = torch.Size(shape), dtype, cuda, requires_grad
        self.device = torch.device("cuda:0" if cuda else "cpu")

    def dim(self):
        return len(self.shape)

    def numel(self):
        return math.prod(self.shape)


def test_kernel_path_decisions(monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (_Fake, torch.Tensor)))
    kp = H.kernel_path
    x, f = _Fake((65536, 128, 3)), _Fake((10,))
    assert kp(x, f) and kp(x, f, _Fake((65536, 128, 3))) and kp(_Fake((3,)), f) and kp(_Fake((0, 3)), f) and kp(x, f, None, False)
    assert not kp(_Fake((5, 3), cuda=False), f) and not kp(torch.zeros(5, 3), torch.ones(4))  # CPU
    assert not kp(_Fake((5, 3), torch.float64), _Fake((10,), torch.float64)) and not kp(_Fake((5, 3), torch.float16), f)
    assert not kp(x, f, _Fake((65536, 128, 1))) and not kp(x, f, _Fake((3,)))  # a diag_cov that broadcasts
    assert not kp(x, _Fake((0,))) and not kp(x, _Fake((10,), requires_grad=True)) and not kp(x, _Fake((2, 5)))
    assert kp(_Fake((2 ** 31 // 63, 3)), f) and not kp(_Fake((2 ** 31 // 63 + 1, 3)), f)  # rows W beyond int32
    assert kp(_Fake((2 ** 31 // 63 + 1, 3)), f, None, False)
    assert kp(_Fake((2, 1)), _Fake((_lib.HARMONIC_MAX_WIDTH // 2,)), None, True) and not kp(_Fake((2, 1)), _Fake((_lib.HARMONIC_MAX_WIDTH // 2 + 1,)), None, False)
    dp = RS.kernel_path
    c = _Fake((10, 128, 128, 150))
    assert dp(c) and dp(c, _Fake((10, 128, 128, 150))) and dp(_Fake((150,)))
    assert not dp(_Fake((4, 150), cuda=False)) and not dp(_Fake((4, 150), torch.float64)) and not dp(_Fake((4, 150), requires_grad=True))
    assert not dp(c, _Fake((10, 128, 128, 1))) and not dp(c, _Fake((10, 128, 128, 150), torch.float64)) and not dp(_Fake((4, 0)))
    assert dp(_Fake((2 ** 31 - 1,))) and not dp(_Fake((2 ** 16, 2 ** 15)))


DEPTHS = C.depth_cases()


def test_stratified_depths_chain_equals_the_reference_s_recording():
    fix = C.fixture()
    assert {c.n for c in DEPTHS} >= {1, 2, 63, 64, 65, 150} and {c.rows for c in DEPTHS if not c.edge} == {1, 3, 257}
    assert {c.form for c in DEPTHS} == set(C.DEPTH_FORMS)
    for case in DEPTHS:
        centers, u = C.depth_centers(case), torch.from_numpy(fix[C.key(case.id, "uniforms")])
        want = torch.from_numpy(fix[C.key(case.id, "depths")])
        keep_c, keep_u = centers.clone(), u.clone()
        assert torch.equal(A.stratified_depths(centers, u), want) and torch.equal(RS.stratified_depths_torch(centers, u), want), case.id
        assert torch.equal(A.stratified_depths(centers.contiguous(), u), want)
        assert torch.equal(centers, keep_c) and torch.equal(u, keep_u) and (case.rows == 1 or case.form != "expand" or centers.stride(0) == 0)
        if case.edge:
            top = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
            assert torch.equal(u, C.edge_uniforms(case)) and float(u.max()) == top < 1.0 and float(u.min()) == 0.0
            lower = torch.cat((centers[..., :1], 0.5 * (centers[..., 1:] + centers[..., :-1])), -1)
            assert torch.equal(want[0::2], lower[0::2])  # u = 0: the lower edge itself
        else:
            torch.manual_seed(C.depth_seed(case))
            assert torch.equal(A.stratified_depths(centers), want)  # the draw of the reference under its seed
    one = torch.tensor([[2.5], [3.5]])
    assert torch.equal(A.stratified_depths(one, torch.rand(2, 1)), one)  # n = 1: c[0] + 0 u


def test_shim_lists_the_patches():
    from pytorch3d_amd import shim

    assert any(m == "pytorch3d.renderer.implicit.harmonic_embedding" and fn is shim._harmonic_embedding for m, _, fn in shim._FUNCTION_PATCHES)
    assert any(m == "pytorch3d.renderer.implicit.raysampling" and fn is shim._stratified_depths for m, _, fn in shim._FUNCTION_PATCHES)
    assert "HarmonicEmbedding.forward" in shim.__doc__ and "_jiggle_within_stratas" in shim.__doc__
