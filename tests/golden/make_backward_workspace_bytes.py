#!/usr/bin/env python3
"""Records tests/golden/backward_workspace_bytes.json: what the three workspace queries of the training backward return, taken from the
build BEFORE the weight-gradient host side described each workspace once (run it against that build: NERF_AMD_LIB=/path/libnerf_amd.so).
No GPU is needed: without one the library sizes its launches for 256 compute units, the MI355X's count, and that is what the table holds.

    NERF_AMD_LIB=/path/to/parent/libnerf_amd.so python tests/golden/make_backward_workspace_bytes.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NETS = {"PROPOSAL": 0, "MIP": 1, "REF": 2}
PRECISIONS = {"F32": 0, "BF16": 1, "BF16_F8": 2}
SIZES = (-1, 0, 1, 32, 33, 2048, 2049, 4097, 16384, 65537, 1048576)


def main():
    from nerf_amd._lib import lib
    table = {"_header": "bytes returned by the workspace queries of the training backward on a device with 256 compute units (MI355X; also the "
                        "library's assumption without a GPU). Keys: 'NET,PRECISION,M' (nerf_amd_ref_backward_workspace_bytes: 'PRECISION,M')."}
    wg, rf, dg = {}, {}, {}
    for p, pc in PRECISIONS.items():
        for M in SIZES:
            rf["%s,%d" % (p, M)] = int(lib.nerf_amd_ref_backward_workspace_bytes(pc, M))
            for n, nc in NETS.items():
                wg["%s,%s,%d" % (n, p, M)] = int(lib.nerf_amd_weight_grads_workspace_bytes(nc, pc, M))
                dg["%s,%s,%d" % (n, p, M)] = int(lib.nerf_amd_density_grad_workspace_bytes(nc, pc, M))
    table["nerf_amd_weight_grads_workspace_bytes"] = wg
    table["nerf_amd_ref_backward_workspace_bytes"] = rf
    table["nerf_amd_density_grad_workspace_bytes"] = dg
    out = os.path.join(ROOT, "tests", "golden", "backward_workspace_bytes.json")
    with open(out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(out, len(wg), len(rf), len(dg))


if __name__ == "__main__":
    main()
