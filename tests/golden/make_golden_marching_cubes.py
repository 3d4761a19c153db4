"""Golden fixture for marching cubes, recorded FROM THE REFERENCE's compiled CPU operator behind its own Python wrapper (build container
only).

    python tests/golden/make_golden_marching_cubes.py   ->  tests/golden/marching_cubes_ref.npz

The generator compiles the reference's csrc/marching_cubes/marching_cubes_cpu.cpp with a binding of a few lines (BINDING below, the
generator's own) through torch.utils.cpp_extension.load into a build directory OUTSIDE the repository, hands it to the unmodified
`pytorch3d.ops.marching_cubes` as `_C.marching_cubes`, and records for every case of tests/marching_cubes_case.py the inputs and the
two lists the wrapper returns on CPU tensors, with return_local_coords False and True (packed, with per-volume sizes), and
err/local/<case>: the reference's own largest |float32 - float64| over the case's local coordinates, its Transform3d chain run in
float64 over the same world vertices.  Nothing of pytorch3d_amd computes anything here (the shim only provides the `_C` module object
the reference imports, and its marching_cubes entry is replaced by the compiled reference operator).

Asserted here:
* the 256-configuration record names one edge per vertex (the table of the case file derives from it), and the edges a configuration
  references are exactly the edges whose endpoints differ;
* "degen": in every volume the first table triangle is degenerate and a later one is not, and the reference returned NEITHER;
* rand579 holds a recorded vertex whose constant coordinate is not an integer;
* the thin, constant, all-inside and all-outside volumes give `[]`, between non-empty ones in mixed_empty;
* the case file's CPU restatement equals every record; on cases without drops the device restatement has the same triangles bit for
  bit in the same order, as many vertices, and strictly ascending ids; on cases with drops it differs by the drop rule alone.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT", "/root/reference")

BINDING = """
#include <torch/extension.h>
std::tuple<at::Tensor, at::Tensor, at::Tensor> MarchingCubesCpu(const at::Tensor& vol, const float isolevel);
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("marching_cubes", &MarchingCubesCpu); }
"""


def reference_operator():
    from torch.utils.cpp_extension import load

    build_dir = os.path.join(tempfile.gettempdir(), "p3d_ref_marching_cubes")
    os.makedirs(build_dir, exist_ok=True)
    binding = os.path.join(build_dir, "binding.cpp")
    with open(binding, "w") as f:
        f.write(BINDING)
    csrc = os.path.join(REFERENCE, "pytorch3d", "csrc")
    ext = load(name="p3d_ref_marching_cubes", sources=[os.path.join(csrc, "marching_cubes", "marching_cubes_cpu.cpp"), binding],
               extra_include_paths=[csrc], build_directory=build_dir, extra_cflags=["-O2"], verbose=False)
    return ext.marching_cubes


def degenerate_flags(C, vol, config):
    """Per table triangle of the one cube of a (2, 2, 2) volume: whether two of its vertices coincide."""
    entries = [C._entry(vol, np.float32(0), 0, 0, 0, e, None)[2] for e in C.table()[config]]
    return [C.degenerate(a, b, c) for a, b, c in zip(entries[0::3], entries[1::3], entries[2::3])]


def find_degenerate_first(C, count=4):
    """Sign configurations with one OUTSIDE corner moved onto the isolevel 0 (it stays outside: 0 < 0 is false), such that the first
    table triangle collapses and a later one does not."""
    found = []
    base = C.config_volumes().numpy()
    for config in range(256):
        for corner in range(8):
            if (config >> corner) & 1 or len(C.table()[config]) < 6:
                continue
            vol = base[config].copy()
            vol[corner >> 2 & 1, corner >> 1 & 1, corner & 1] = 0.0
            flags = degenerate_flags(C, vol, config)
            if flags[0] and not all(flags[1:]):
                found.append(torch.from_numpy(vol))
                break
        if len(found) == count:
            return torch.stack(found)
    raise AssertionError("no configuration with a degenerate first triangle")


def pack(lists):
    verts, faces = lists
    nv = np.array([len(v) for v in verts], np.int64)
    nf = np.array([len(f) for f in faces], np.int64)
    assert all((a == 0) == (b == 0) for a, b in zip(nv, nf))
    vs = [v for v in verts if torch.is_tensor(v)]
    fs = [f for f in faces if torch.is_tensor(f)]
    assert all(v.dtype == torch.float32 and v.dim() == 2 for v in vs) and all(f.dtype == torch.int64 and f.dim() == 2 for f in fs)
    return (torch.cat(vs).numpy() if vs else np.zeros((0, 3), np.float32), torch.cat(fs).numpy() if fs else np.zeros((0, 3), np.int64), nv, nf)


def main():
    import marching_cubes_case as C
    import run_reference_suite as rrs

    op = reference_operator()
    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    mod = shim.install(REFERENCE)
    mod.marching_cubes = op  # the reference's own compiled CPU operator, not this package's
    import importlib

    ref = importlib.import_module("pytorch3d.ops.marching_cubes")
    transforms = importlib.import_module("pytorch3d.transforms")
    assert ref._C.marching_cubes is op and not getattr(ref.marching_cubes, "__p3d_amd__", False)

    data = {}
    C._FIXTURE, C._TABLE = data, None

    def record(name, vol, iso):
        data[name + "/vol"], data[name + "/iso"] = vol.contiguous().numpy(), np.float64(float("nan") if iso is None else iso)
        worst = 0.0
        for local in (False, True):
            lists = ref.marching_cubes(C.strided(name, vol), iso, return_local_coords=local)
            key = "%s/%d/" % (name, local)
            data[key + "verts"], data[key + "faces"], data[key + "nv"], data[key + "nf"] = pack(lists)
        D, H, W = vol.shape[1:]
        for world, local32 in zip(*[C.expected(name, k)[0] for k in (False, True)]):
            if torch.is_tensor(world):
                chain = (transforms.Translate(x=1.0, y=1.0, z=1.0, dtype=torch.float64)
                         .scale((torch.tensor([[W, H, D]], dtype=torch.float64) - 1) * 0.5).inverse())
                local64 = chain.transform_points(world.double()[None])[0]
                diff = (local32.double() - local64).abs()
                worst = max(worst, float(diff[~diff.isnan()].max()) if (~diff.isnan()).any() else 0.0)
        data["err/local/" + name] = np.float64(worst)
        print("%-12s %-16s V %6d  F %6d  reference's local error %.3g" % (name, tuple(vol.shape), int(data[name + "/0/nv"].sum()),
                                                                         int(data[name + "/0/nf"].sum()), worst))

    record("cfg256", *C.build_inputs("cfg256"))
    table = C.table()
    assert len(table) == 256 and max(len(t) for t in table) <= 15 and all(len(t) % 3 == 0 for t in table)
    assert all(set(t) == C.crossed_edges(c) for c, t in enumerate(table)), "referenced edges are not the crossed edges"
    degenerate_first = find_degenerate_first(C)
    for name in C.cases()[1:]:
        record(name, *C.build_inputs(name, degenerate_first))

    # what the case file's header promises
    assert data["degen/0/nf"].tolist() == [0] * len(degenerate_first), "the reference kept a triangle behind a degenerate one"
    for vol in degenerate_first:
        flags = degenerate_flags(C, vol.numpy(), sum(int(vol.reshape(-1)[i] < 0) << i for i in range(8)))
        assert flags[0] and not all(flags[1:])
    world = data["rand579/0/verts"]
    integer = world == np.round(world)
    assert ((~integer).sum(1) >= 2).any(), "no recorded vertex with a constant coordinate that is not an integer"
    assert all(int(data[n + "/0/nf"].sum()) == 0 for n in ("thin_d", "thin_h", "thin_w"))
    nf = data["mixed_empty/0/nf"].tolist()
    assert nf[0] > 0 and nf[1:4] == [0, 0, 0] and nf[4] > 0
    assert data["isonone/0/nf"].min() > 0 and data["naninf/0/nf"].min() > 0 and data["snap/0/nf"].min() > 0

    drops = []
    for name in C.cases():
        for local in (False, True):
            wrong = C.misses(C.restated(name, local, "cpu"), C.expected(name, local), name, C.tolerance(name, local))
            assert wrong == [], wrong
        vol, iso = C.inputs(name)
        assert C.tie_misses(name) == [], C.tie_misses(name)
        if C.has_drops(name):
            drops.append(name)
        for v in vol:
            level = ((v.max() + v.min()) / 2).item() if iso is None else iso
            ids = C.restate_device_one(v.numpy(), level)[2]
            assert bool((ids[1:] > ids[:-1]).all()), name
    assert "degen" in drops and "snap" in drops and "cfg256" not in drops and "rand579" not in drops, drops
    np.savez_compressed(C.FIXTURE, **data)
    print("cases with drops:", drops)
    print("wrote %s: %d cases, %d bytes" % (C.FIXTURE, len(C.cases()), os.path.getsize(C.FIXTURE)))


if __name__ == "__main__":
    main()
