"""Writes csrc/marching_cubes_tables.h from the record of the 256 sign configurations in tests/golden/marching_cubes_ref.npz.

    python pytorch3d_amd/csrc/make_marching_cubes_tables.py

The record (tests/golden/make_golden_marching_cubes.py) holds what the reference's compiled CPU operator returned for the 256 volumes
(2, 2, 2) of +-1 at isolevel 0, volume c having -1 at corner i = x + 2 y + 4 z iff bit i of c is set.  Every vertex of such a mesh is
the midpoint of one cube edge: the coordinate at 0.5 names the axis, the other two the edge's low corner.  Read triangle by triangle
that gives the table in the reference's order and this project's numbering: entry = 8 * axis + corner, 255 behind the last.
tests/test_cpu_marching_cubes.py derives the same entries again and compares them with the compiled header one by one.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "..", "..", "tests", "golden", "marching_cubes_ref.npz")
HEADER = os.path.join(HERE, "marching_cubes_tables.h")

TEXT = """// marching_cubes_tables.h -- the triangle table of marching cubes in this project's numbering.  WRITTEN BY make_marching_cubes_tables.py
// (next to this file) from the recorded meshes of the 256 sign configurations; do not edit.
//   corner i of a cube = its low corner moved by (i & 1, i >> 1 & 1, i >> 2 & 1); configuration bit i: corner i is inside;
//   entry = 8 * axis + corner: the edge from `corner` (whose axis bit is 0) one step along axis 0 = x, 1 = y, 2 = z; 255: no entry.
// Functions instead of arrays: a constexpr array inside a __host__ __device__ function is the one spelling both sides can index.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define P3D_MC_HD __host__ __device__ inline
#else
#define P3D_MC_HD inline
#endif

namespace p3d {

// triangles of a configuration, 0..5
P3D_MC_HD uint8_t mc_triangle_count(int config) {
  constexpr uint8_t counts[256] = {
%s};
  return counts[config];
}

// entry k (0..15) of a configuration's row: 3 * mc_triangle_count(config) entries, then 255
P3D_MC_HD uint8_t mc_table_entry(int config, int k) {
  constexpr uint8_t entries[256][16] = {
%s};
  return entries[config][k];
}

}  // namespace p3d
"""


def table():
    with np.load(FIXTURE) as z:
        verts, faces, nv, nf = (z["cfg256/0/" + k] for k in ("verts", "faces", "nv", "nf"))
    rows, v0, f0 = [], 0, 0
    for config in range(256):
        tri = verts[v0:v0 + nv[config]][faces[f0:f0 + nf[config]].reshape(-1)]
        v0, f0 = v0 + nv[config], f0 + nf[config]
        row = []
        for p in tri.tolist():
            axis = [a for a in range(3) if p[a] == 0.5]
            assert len(axis) == 1 and all(c in (0.0, 0.5, 1.0) for c in p), (config, p)
            row.append(8 * axis[0] + sum(int(p[a]) << a for a in range(3) if a != axis[0]))
        assert len(row) % 3 == 0 and len(row) <= 15, config
        rows.append(row)
    return rows


def main():
    rows = table()
    counts = "".join("      " + ", ".join("%d" % (len(r) // 3) for r in rows[k:k + 32]) + ",\n" for k in range(0, 256, 32))
    entries = "".join("      {" + ", ".join("%3d" % e for e in r + [255] * (16 - len(r))) + "},\n" for r in rows)
    with open(HEADER, "w") as f:
        f.write(TEXT % (counts, entries))
    print("wrote", HEADER)


if __name__ == "__main__":
    main()
