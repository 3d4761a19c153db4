#!/usr/bin/env python
"""The reference's own tests/test_face_areas_normals.py through tests/run_reference_suite.py, in a process of its own.

    python tests/ref_face_areas_normals_case.py --out FILE [--torch-formulation]

--torch-formulation switches the dispatch of pytorch3d_amd/_aux_ops.py off first: every input takes the torch formulation, which is
what ran before csrc/normals.hip existed -- the outcome per case that the kernels must not fall behind
(tests/test_gpu_mesh_normals.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    args = sys.argv[1:]
    if "--torch-formulation" in args:
        args.remove("--torch-formulation")
        from pytorch3d_amd import _aux_ops

        _aux_ops.fused_face_areas_normals = lambda *a: False
    import run_reference_suite as rrs

    sys.argv = ["run_reference_suite.py"] + args + ["test_face_areas_normals"]
    rrs.main()


if __name__ == "__main__":
    main()
