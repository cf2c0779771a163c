"""What the plan kernels of csrc/kernels/helmholtz_fused.hip are launched with, for comparing two builds of the library:
  rocprofv3 --kernel-trace -d DIR -- python3 profiles/tools/launch_geometry.py run DIR      (once per build, no counters)
  python3 profiles/tools/launch_geometry.py compare DIR_OLD DIR_NEW
`run` builds one plan of every form (lane form with and without PRE; helm_patch_kernel on 32- and 64-element patches with and
without MODE=1, affine and with non-temporal loads; helm_mfma_kernel staged and unstaged; op_patch_kernel on 32- and 64-element
patches; op_mfma_kernel), applies each once -- the fused ones in both vector orderings -- and saves the results to DIR/outputs.npz
and, to DIR/plans.txt, the lines it prints: kernel() of every plan and, for the fused ones, the four byte figures (algorithmic, as
laid out, affine, native ordering; the single operators expose none -- what theirs decides, the NT flag, is part of kernel()).
`compare` reads the two traces (the rocpd database rocprofv3 leaves under DIR) and prints, dispatch by dispatch, kernel name,
grid, workgroup and LDS bytes of both builds, whether they are the same, whether the saved results are (np.array_equal) and
whether the plan lines are."""
import csv
import os
import sqlite3
import sys
from pathlib import Path

import numpy as np

KNOBS = ("CUDDH_PLAN_AFFINE", "CUDDH_PLAN_STREAMING", "CUDDH_HELM_PE", "CUDDH_HELM_LANE", "CUDDH_HELM_PRE", "CUDDH_HELM_PAIR_MASS", "CUDDH_HELM_MFMA_STAGE",
         "CUDDH_OP_PE")
# (label, n_basis, knobs)
FUSED = [("lane", 4, {"CUDDH_HELM_LANE": "1", "CUDDH_HELM_PRE": "0"}),
         ("lane NT", 4, {"CUDDH_HELM_LANE": "1", "CUDDH_PLAN_STREAMING": "1"}),
         ("lane PRE", 4, {"CUDDH_HELM_LANE": "1", "CUDDH_HELM_PRE": "1"}),
         ("patch 32 MODE=1", 3, {"CUDDH_HELM_LANE": "0", "CUDDH_HELM_PE": "32"}),
         ("patch 32", 3, {"CUDDH_HELM_LANE": "0", "CUDDH_HELM_PE": "32", "CUDDH_HELM_PAIR_MASS": "0"}),
         ("patch 64 MODE=1", 3, {"CUDDH_HELM_LANE": "0", "CUDDH_HELM_PE": "64"}),
         ("patch 64", 3, {"CUDDH_HELM_LANE": "0", "CUDDH_HELM_PE": "64", "CUDDH_HELM_PAIR_MASS": "0"}),
         ("patch affine", 4, {"CUDDH_PLAN_AFFINE": "1"}),
         ("patch n_basis 5", 5, {}),
         ("mfma staged", 6, {}),
         ("mfma unstaged", 6, {"CUDDH_HELM_MFMA_STAGE": "0"})]
OPS = [("op patch 32", 4, {"CUDDH_OP_PE": "32"}), ("op patch 64", 4, {"CUDDH_OP_PE": "64"}), ("op mfma", 6, {})]


def run(out_dir: Path):
    import torch

    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
    import cuddhelmholtz_amd as cd

    dev = torch.device("cuda:0")
    cd.use_torch_stream()
    mesh = cd.Mesh2D.uniform_rect(13, -1.0, 1.0, 13, -1.0, 1.0)
    faces = mesh.boundary_edges()
    saved, lines = {}, []

    def case(nb, knobs):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ["CUDDH_PLAN_AFFINE"] = "0"  # the general-geometry layout unless the case says otherwise
        os.environ.update(knobs)
        fem = cd.H1Space(mesh, cd.Basis(nb))
        g = torch.Generator(device="cpu").manual_seed(nb)
        return fem, (0.5 + torch.rand(fem.size(), generator=g, dtype=torch.float64)).to(dev), torch.randn(2 * fem.size(), generator=g, dtype=torch.float64).to(dev)

    for label, nb, knobs in FUSED:
        fem, a2, x = case(nb, knobs)
        fs = cd.FaceSpace(fem, faces)
        A = cd.HelmholtzOperator(7.0, a2, torch.ones(fs.size(), dtype=torch.float64, device=dev), fem, fs)
        y, z, zy = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
        A.action(x, y)
        A.to_native(x, z)
        A.action_native(z, zy)
        torch.cuda.synchronize()
        lines.append(f"{label}: {A.kernel()} | bytes_per_apply 0-3: {A.bytes_per_apply()} {A.bytes_per_apply(True)} {A.bytes_affine()} {A.bytes_native()}")
        saved[label + " | reference ordering"], saved[label + " | native ordering"] = y.cpu().numpy(), zy.cpu().numpy()
    for label, nb, knobs in OPS:
        fem, a2, x = case(nb, knobs)
        n = fem.size()
        for name, op in (("stiffness", cd.StiffnessMatrix(fem)), ("weighted mass", cd.MassMatrix(fem, a2))):
            y = torch.zeros(n, dtype=torch.float64, device=dev)
            op.action(x[:n], y)
            op.action(0.5, x[:n], y)  # the accumulating form
            torch.cuda.synchronize()
            lines.append(f"{label}, {name}: {op.kernel()}")
            saved[f"{label} | {name}"] = y.cpu().numpy()
    np.savez(out_dir / "outputs.npz", **saved)
    (out_dir / "plans.txt").write_text("\n".join(lines) + "\n")
    print(*lines, sep="\n")


def dispatches(trace_dir: Path):
    dbs = sorted(trace_dir.rglob("*.db"))
    if dbs:
        rows = sqlite3.connect(dbs[-1]).execute("select name, grid_x, workgroup_x, lds_size from kernels order by start").fetchall()
    else:  # a rocprofv3 that writes CSV
        with open(sorted(trace_dir.rglob("*kernel_trace.csv"))[-1], newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        rows = [(r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"]), int(r["LDS_Block_Size"])) for r in rows]
    return [r for r in rows if any(k in r[0] for k in ("helm_", "op_patch", "op_mfma", "op_border", "native_kernel"))]


def compare(old_dir: Path, new_dir: Path):
    old, new = dispatches(old_dir), dispatches(new_dir)
    print(f"{len(old)} dispatches of the plan kernels before, {len(new)} after")
    print("dispatch | kernel | grid workgroup lds_bytes before | after | same")
    same = 0
    for i in range(max(len(old), len(new))):
        a, b = (old[i] if i < len(old) else None), (new[i] if i < len(new) else None)
        same += a == b
        print(f"{i} | {(a or b)[0]} | {' '.join(map(str, a[1:])) if a else 'MISSING'} | {' '.join(map(str, b[1:])) if b else 'MISSING'}"
              f"{'' if not (a and b) or a[0] == b[0] else ' of ' + b[0]} | {'same' if a == b else 'DIFFERS'}")
    print(f"{same} of {max(len(old), len(new))} dispatches: same kernel, grid, workgroup and LDS bytes")
    ya, yb = np.load(old_dir / "outputs.npz"), np.load(new_dir / "outputs.npz")
    equal = [k for k in ya.files if k in yb.files and np.array_equal(ya[k], yb[k])]
    for k in sorted(set(ya.files) | set(yb.files)):
        print(f"result of {k}: {'bitwise equal' if k in equal else 'DIFFERS'}")
    print(f"{len(equal)} of {len(set(ya.files) | set(yb.files))} results: np.array_equal")
    pa, pb = (old_dir / "plans.txt").read_text().splitlines(), (new_dir / "plans.txt").read_text().splitlines()
    for i in range(max(len(pa), len(pb))):
        a, b = (pa[i] if i < len(pa) else "MISSING"), (pb[i] if i < len(pb) else "MISSING")
        print(f"plan {a} | {'same' if a == b else 'DIFFERS, after: ' + b}")
    print(f"{sum(a == b for a, b in zip(pa, pb))} of {max(len(pa), len(pb))} plans: same kernel() and byte figures")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(Path(sys.argv[2]))
    else:
        compare(Path(sys.argv[2]), Path(sys.argv[3]))
