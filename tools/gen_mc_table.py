#!/usr/bin/env python3
"""Print the marching-cubes case table of nice_slam_amd/csrc/nsr_kernels.h (kMcTable) from the construction in
tests/mesh_reference.py::mc_table: per case, the triangle count, then up to five triangles as cell-edge triples."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from mesh_reference import mc_table  # noqa: E402


def main():
    rows = []
    for tris in mc_table():
        flat = [len(tris)] + [e for t in tris for e in t]
        flat += [0] * (16 - len(flat))
        rows.append("{" + ",".join(str(x) for x in flat) + "}")
    print("constexpr unsigned char kMcTable[256][16] = {")
    for i in range(0, 256, 4):
        print("    " + ", ".join(rows[i:i + 4]) + ",")
    print("};")


if __name__ == "__main__":
    main()
