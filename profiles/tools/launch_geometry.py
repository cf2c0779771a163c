"""What the plan kernels of csrc/kernels/helmholtz_fused.hip are launched with, for comparing two builds of the library:
  rocprofv3 --kernel-trace -d DIR -- python3 profiles/tools/launch_geometry.py run DIR      (once per build, no counters)
  python3 profiles/tools/launch_geometry.py compare DIR_OLD DIR_NEW
`run` builds one plan of every form (lane form with and without PRE; helm_patch_kernel on 32- and 64-element patches with and
without MODE=1, affine and with non-temporal loads; helm_mfma_kernel staged and unstaged; op_patch_kernel on 32- and 64-element
patches; op_mfma_kernel), applies each once -- the fused ones in both vector orderings -- and saves the results to DIR/outputs.npz
and, to DIR/plans.txt, the lines it prints: kernel() of every plan and, for the fused ones, the four byte figures (algorithmic, as
laid out, affine, native ordering; the single operators expose none -- what theirs decides, the NT flag, is part of kernel()).
`compare` reads the two traces (the rocpd database rocprofv3 leaves under DIR) and prints, dispatch by dispatch, kernel name,
grid, workgroup and LDS bytes of both builds, whether they are the same (names literally, after the declared renames in RENAMED
have been applied to the build before), whether the saved results are (np.array_equal) and whether the plan lines are.
`run-ddh DIR` does the same for the DDH local-solve kernels of csrc/kernels/ddh.hip (the list DDH below: one plan per resolved
kernel, sweep form, chain order, with and without time grids and RK4); `compare` then lists every ddh_* dispatch, the plan
creation's check kernels included."""
import csv
import os
import re
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


# DDH plans, one per resolved form of csrc/kernels/ddh.hip: (label, n_basis, elements per side, block, label block, precision, kernel,
# creation keywords, setters); four subdomains each
DDH_GRIDS = np.array([1, 2, 1, 1], dtype=np.int32)
DDH = [("kernel 1", 4, 8, None, None, "f32", 1, {}, ()),
       ("kernel 1 f64 grids", 4, 8, None, None, "f64", 1, {"time_step": DDH_GRIDS}, ()),
       ("kernel 1 n_basis 5 block 6 (1024-thread form)", 5, 12, 6, None, "f32", 1, {}, ()),
       ("kernel 2", 4, 8, None, None, "f32", 2, {}, ()),
       ("kernel 3", 4, 8, None, None, "f32", 3, {}, ()),
       ("kernel 3 f64", 4, 8, None, None, "f64", 0, {}, ()),
       ("kernel 4", 4, 8, None, None, "f32", 4, {}, ()),
       ("kernel 5 form 1", 4, 8, None, None, "f32", 0, {}, ()),
       ("kernel 5 form 1 grids", 4, 8, None, None, "f32", 0, {"time_step": DDH_GRIDS}, ()),
       ("kernel 5 form 2 pinned", 4, 8, None, None, "f32", 0, {}, (("set_sweep_form", 2),)),
       ("kernel 5 form 2 paired", 4, 8, None, None, "f32", 0, {}, (("set_sweep_form", 2), ("set_chain_order", 2))),
       ("kernel 5 form 3 pinned", 4, 8, None, None, "f32", 0, {}, (("set_sweep_form", 3),)),
       ("kernel 6", 8, 4, None, None, "f64", 0, {}, ()),
       ("kernel 6 f32", 8, 4, None, None, "f32", 6, {}, ()),
       ("kernel 7", 8, 4, None, None, "f32", 0, {}, ()),
       ("kernel 8", 4, 8, None, None, "f64", 8, {}, ()),
       ("kernel 9", 4, 8, None, 4, "f32", 0, {}, ()),
       ("kernel 9 f64 grids RK4", 4, 8, None, 4, "f64", 9, {"time_ratios": DDH_GRIDS, "integrator": "rk4"}, ()),
       ("kernel 10", 5, 6, None, 3, "f32", 0, {}, ()),
       ("kernel 11", 4, 16, 8, None, "f32", 0, {}, ()),
       ("kernel 11 grids, last copy", 4, 16, 8, None, "f32", 0, {"time_step": DDH_GRIDS}, (("set_owner_rule", True),)),
       ("kernel 12", 5, 8, 4, None, "f32", 12, {}, ()),
       ("kernel 12 last copy", 5, 8, 4, None, "f32", 12, {}, (("set_owner_rule", True),)),
       ("kernel 13 n_basis 4", 4, 8, None, None, "f32", 13, {}, ()),
       ("kernel 13 n_basis 4 grids", 4, 8, None, None, "f32", 13, {"time_step": DDH_GRIDS}, ()),
       ("kernel 13 n_basis 5", 5, 8, 4, None, "f32", 13, {}, ()),
       ("kernel 13 n_basis 5 grids", 5, 8, 4, None, "f32", 13, {"time_step": DDH_GRIDS}, ()),
       ("kernel 1 RK4", 4, 8, None, None, "f32", 1, {"integrator": "rk4"}, ()),
       ("kernel 2 RK4 (auto, f64)", 4, 8, None, None, "f64", 0, {"integrator": "rk4"}, ()),
       ("kernel 5 RK4", 4, 8, None, None, "f32", 0, {"integrator": "rk4"}, ()),
       ("kernel 5 RK4 grids", 4, 8, None, None, "f32", 0, {"integrator": "rk4", "time_step": DDH_GRIDS}, ()),
       ("kernel 8 RK4", 4, 8, None, None, "f64", 8, {"integrator": "rk4"}, ())]


def run_ddh(out_dir: Path):
    """One plan per entry of DDH: its local solves over all subdomains, over two ranges, listed while holding issue priority, and
    without sources (the form without x); the traces go to DIR/outputs.npz, kernel / sweep form / chain order to DIR/plans.txt."""
    import math

    import torch

    sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
    import cuddhelmholtz_amd as cd

    dev = torch.device("cuda:0")
    cd.use_torch_stream()
    saved, lines = {}, []
    for label, nb, nx, block, label_block, precision, kernel, kw, setters in DDH:
        fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
        omega, h_a = 2 * math.pi * nx / 10, np.ones(fem.size())
        if label_block:
            e = np.arange(nx * nx)
            labels = ((e % nx) // label_block + (nx // label_block) * ((e // nx) // label_block)).astype(np.int32)
            F = cd.DDH.from_labels(omega, h_a, fem, labels, precision=precision, kernel=kernel, **kw)
        else:
            F = cd.DDH(omega, h_a, fem, nx, nx, precision=precision, kernel=kernel, block=block, **kw)
        for setter, arg in setters:
            getattr(F, setter)(arg)
        F.set_wh_iters(1)
        nd = F.info()["n_domains"]
        g = torch.Generator(device="cpu").manual_seed(nb)
        f = torch.randn(2 * fem.size(), generator=g, dtype=torch.float64).to(dev)
        lam = torch.randn(F.size(), generator=g, dtype=torch.float64).to(F.trace_dtype).to(dev)
        out = [torch.zeros_like(lam) for _ in range(4)]
        F.local_traces(0, nd, f, lam, out[0])
        F.local_traces(0, nd - 1, f, lam, out[1])
        F.local_traces(nd - 1, nd, f, lam, out[1])
        F.set_wave_priority(True)
        F.local_traces_listed(torch.tensor([2, 0, 3], dtype=torch.int32, device=dev), f, lam, out[2])
        F.set_wave_priority(False)
        F.local_traces(0, nd, None, lam, out[3])
        torch.cuda.synchronize()
        lines.append(f"{label}: kernel {F.info()['kernel']} sweep form {F.sweep_form()} chain order {F.chain_order()} integrator {F.integrator()[0]} "
                     f"time ratios {' '.join(map(str, F.time_ratios()))}")
        for name, t in zip(("all", "two ranges", "listed, priority", "no sources"), out):
            saved[f"{label} | {name}"] = t.cpu().numpy()
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
    return [r for r in rows if any(k in r[0] for k in ("helm_", "op_patch", "op_mfma", "op_border", "native_kernel", "ddh_"))]


# kernels whose symbol changed: (pattern, replacement) pairs applied in this order to the names of the build before, which are then
# compared literally.  ddh_element_lane5_kernel<F, H, L, ..> became ddh_element_lane_kernel<5, F, H, L, false, ..>, and
# ddh_element_lane_kernel<F, H, L, P, ..> got NB = 4 as its first argument.
RENAMED = ((r"ddh_element_lane5_kernel<(\w+, \w+, \w+)", r"ddh_element_lane_kernel<5, \1, false"),
           (r"ddh_element_lane_kernel<((?:true|false), \w+, \w+, \w+)", r"ddh_element_lane_kernel<4, \1"))


def renamed(row):
    name = row[0]
    for pattern, repl in RENAMED:
        name = re.sub(pattern, repl, name)
    return (name, *row[1:])


def compare(old_dir: Path, new_dir: Path):
    old, new = [renamed(r) for r in dispatches(old_dir)], dispatches(new_dir)
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
    elif sys.argv[1] == "run-ddh":
        run_ddh(Path(sys.argv[2]))
    else:
        compare(Path(sys.argv[2]), Path(sys.argv[3]))
