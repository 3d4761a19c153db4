"""The clipping cases without a GPU: the float64 restatement against the fixture's truth, the float32 restatement through the gates
(they are E_ref-derived, so the reference's own arithmetic passes them), the branches and shapes the cases promise, and five
arithmetic-only mistakes that the gates refuse.  Cases, restatement and gates: tests/clip_case.py; fixture:
tests/golden/clip_cases_ref.npz."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_case as C  # noqa: E402

CASES, CONVERT = C.cases(), C.convert_cases()


def test_float64_restatement_is_the_fixture_truth_on_every_case():
    fix = C.fixture()
    assert os.path.getsize(C.FIXTURE) < 1_000_000
    for case in CASES + CONVERT:
        t = C.truth(case)  # asserts 1e-12 of each row's scale on the rows held, and equal tables
        for q in C.float_quantities(case):
            assert (t[q] is None) == (C.key(case.id, q) not in fix), (case.id, q)
    for q in C.BLOCK_QUANTITIES + C.SAMPLE_QUANTITIES:
        assert 0.0 < C.e_ref(q) < 5e-5, q
    assert C.e_ref("grad_face_verts") < 2e-6 and C.e_ref("face_verts") < 5e-7


def test_float32_restatement_lies_within_the_gates():
    assert C.failures(CASES + CONVERT, C.torch_impl()) == []


def test_every_branch_combination_is_reached():
    want = {(i1, kase, persp) for i1, kase in C.BRANCH_COMBOS for persp in (True, False)}
    assert C.branches(C.case_by_id("branch-persp")) | C.branches(C.case_by_id("branch-flat")) == want
    assert C.branches(C.case_by_id("seeded-persp")) | C.branches(C.case_by_id("seeded-flat")) == want
    for case in CASES:  # a case-4 face takes two consecutive faces that name each other
        t = C.truth(case)
        nbr = t[C.TABLES[4]]
        if nbr is not None:
            pair = np.nonzero(nbr >= 0)[0]
            assert np.array_equal(nbr[nbr[pair]], pair)
    rows = C.truth(C.case_by_id("seeded-persp"))["barycentric_conversion"].shape[0]
    assert 380 <= rows <= 520  # a wave's 1024 samples over these fill the 182-slot table past 118 several times


def test_onplane_cases_hold_what_they_promise():
    fix = C.fixture()
    for cid in ("onplane-persp", "onplane-flat"):
        case = C.case_by_id(cid)
        fv = C.inputs(case)[0]
        assert int((fv[:, :, 2] == 0.25).sum()) >= 12
        t = C.truth(case)
        conv = t["barycentric_conversion"]
        assert set(np.unique(conv)) == {0.0, 0.5, 1.0}  # every w is exactly 0, 1/2 or 1
        assert t[C.TABLES[2]].tolist().count(12) == 1  # the face with all three vertices on the plane is kept whole
        got = C.run_clip(C.torch_impl(), case)  # float32: exact arithmetic, the same bits as the reference's float32 and as the truth
        assert C.same_bits(got["face_verts"], fix[C.key(cid, "f32_face_verts")]) and C.same_bits(got["barycentric_conversion"], fix[C.key(cid, "f32_barycentric_conversion")])
        for q in C.float_quantities(case):
            assert np.array_equal(got[q], t[q]), (cid, q)


def test_cull_cases_tell_the_two_readings_of_a_plane_apart():
    t = C.truth(C.case_by_id("cull-only"))
    kept = set(t[C.TABLES[2]].tolist())
    assert kept == {f for f in range(18) if f % 3 != 0}  # per plane: the reference's reading culls face 3 pl, the intended one 3 pl + 2
    assert t["barycentric_conversion"] is None and t[C.TABLES[3]] is None
    fv = C.inputs(C.case_by_id("cull-only"))[0]
    planes = [C.SIX[k] for k in ("left", "right", "top", "bottom", "znear", "zfar")]
    for pl, val in enumerate(planes):
        beyond = (lambda x: x > val) if pl & 1 else (lambda x: x < val)
        assert bool(beyond(fv[3 * pl, pl >> 1, :]).all()) and not bool(beyond(fv[3 * pl, :, pl >> 1]).all())
        assert bool(beyond(fv[3 * pl + 2, :, pl >> 1]).all()) and not bool(beyond(fv[3 * pl + 2, pl >> 1, :]).all())
    off, six = C.truth(C.case_by_id("cull-off")), C.truth(C.case_by_id("cull-six"))
    assert off["face_verts"].shape[0] > six["face_verts"].shape[0]  # cull=False with the planes set keeps what they would take
    bad = C.inputs(C.case_by_id("cull-nonfinite"))[0][list(C.NONFINITE_FACES)]
    assert torch.isnan(bad[:, :, 2]).any() and torch.isinf(bad[:, :, 2]).any() and torch.isnan(bad[:, :, 0]).any() and torch.isinf(bad[:, :, 0]).any()
    fine = C.inputs(C.case_by_id("cull-nonfinite"))[0]
    assert torch.isfinite(fine[12]).all() and torch.isfinite(fine[25]).all()


def test_mesh_and_scan_cases_hold_what_they_promise():
    t = C.truth(C.case_by_id("meshes-empties"))
    first, count = t[C.TABLES[0]], t[C.TABLES[1]]
    Fc = t["face_verts"].shape[0]
    assert count[0] == 0 and count[2] == 0 and count[4] == 0 and count[5] == 0 and first[4] == Fc and first[5] == Fc and count.sum() == Fc
    assert C.inputs(C.case_by_id("meshes-empties"))[1][-1] == 12  # first[n] == F
    t = C.truth(C.case_by_id("meshes-mesh-removed"))
    assert t[C.TABLES[1]][1] == 0 and t[C.TABLES[1]][0] > 0 and t[C.TABLES[1]][2] > 0
    t = C.truth(C.case_by_id("meshes-nothing-left"))
    assert t["face_verts"].shape == (0, 3, 3) and t[C.TABLES[2]].shape == (0,) and not t[C.TABLES[1]].any() and t["barycentric_conversion"] is None
    assert not t["grad_face_verts/both"].any()
    assert C.truth(C.case_by_id("meshes-one"))[C.TABLES[0]].shape == (1,)
    for F in (1025, 2049):
        t = C.truth(C.case_by_id("scan-F%d" % F))
        c2u, nbr = t[C.TABLES[2]], t[C.TABLES[4]]
        at = np.nonzero(c2u == 1023)[0]
        assert at.size == 2 and nbr[at[0]] == at[1] and 1024 not in c2u  # delta 2 on the last row of a block, delta 0 on the next row
    assert [c.arg for c in CASES if c.kind == "scan"] == list(C.SCAN_F) and {c.S for c in CONVERT} == set(C.CONVERT_S)


def test_convert_patterns_hold_what_they_promise():
    base = C.truth(C.case_by_id("seeded-persp"))
    conv_idx = base[C.TABLES[3]]
    for case in CONVERT[:-1]:
        keys = C.convert_inputs(case)[0].reshape(-1).numpy()
        assert keys.min() >= -1 and keys.max() < conv_idx.size  # inside the tables
        rows = np.where(keys >= 0, conv_idx[np.maximum(keys, 0)], -1)
        if case.pattern == "onerow":
            assert rows.min() == rows.max() >= 0
        if case.pattern == "tworows":
            assert set(rows.tolist()) <= {5, rows.max()} and rows[0] == 5 and (case.S == 1 or rows[1] != 5)
        if case.pattern == "fresh":
            assert all(len(set(rows[i:i + 64].tolist())) == min(64, case.S - i) for i in range(0, case.S, 64)) and rows.min() >= 0
        if case.pattern == "kept":
            assert (rows == -1).all() and (keys >= 0).all()
        if case.pattern == "random" and case.S >= 257:
            assert 0.15 < (keys == -1).mean() < 0.35 and (rows >= 0).any() and ((rows == -1) & (keys >= 0)).any()
    wave = np.where(C.convert_inputs(C.case_by_id("convert-S4096-random"))[0].reshape(-1).numpy()[:1024] >= 0, 1, 0)
    keys = C.convert_inputs(C.case_by_id("convert-S4096-random"))[0].reshape(-1).numpy()[:1024]
    assert len(set(conv_idx[keys[keys >= 0]].tolist())) > 2 * 118 and wave.any()  # one wave's samples: more distinct rows than two flushes hold
    assert C.truth(C.case_by_id("convert-noconv"))["grad_conversion"] is None


def _old_gate_lets_through(got, want):
    """tests/test_gpu_clip.py's gradient gate: rtol 2e-3 plus atol 1e-4 max(1, max|ref|) over the whole case."""
    return bool(np.allclose(got, want, rtol=2e-3, atol=1e-4 * max(1.0, float(np.abs(want).max()))))


# mistake -> does test_gpu_clip.py's gate accept it on the seeded cases (both gradients into face_verts and into the conversion, as
# that test sums them)?  It sees the fixture's gradient of a 60-face case only, never the samples, so a mistake in the sample
# gradient cannot reach it at all.
OLD_GATE_ACCEPTS = {"keep_w3": False, "swap_w_persp": False, "drop_g2_second": False, "conv_untransposed": True, "drop_gconv_w2": False}


@pytest.mark.parametrize("wrong", C.WRONGS)
def test_arithmetic_mistakes_are_refused_by_the_gates(wrong):
    subset = [c for c in CASES if c.kind in ("branch", "seeded", "onplane")] + [c for c in CONVERT if c.S in (65, 257)]
    bad = C.failures(subset, C.torch_impl(wrong))
    assert bad, wrong
    assert not any(q in C.TABLES or q in ("face_verts", "barycentric_conversion", "bary_unclipped", "pix_to_face_unclipped") for _, q, _, _ in bad)  # arithmetic of the gradients only
    if wrong == "swap_w_persp":
        assert all(C.case_by_id(cid).frustum["perspective_correct"] for cid, _, _, _ in bad if isinstance(C.case_by_id(cid), C.Case))
    if wrong == "conv_untransposed":
        assert {q for _, q, _, _ in bad} == {"grad_bary_clipped"}
    if wrong == "drop_gconv_w2":
        assert {q for _, q, _, _ in bad} <= {"grad_face_verts/conv", "grad_face_verts/both", "grad_face_verts_from_samples"}
    accepted = []
    for cid in ("seeded-persp", "seeded-flat"):
        case = C.case_by_id(cid)
        got, want = C.run_clip(C.torch_impl(wrong), case), C.truth(case)
        accepted.append(_old_gate_lets_through(got["grad_face_verts/both"], want["grad_face_verts/both"]))
    print(wrong, "old gate accepts on", accepted)
    assert all(accepted) == OLD_GATE_ACCEPTS[wrong], (wrong, accepted)
