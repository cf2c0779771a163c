"""Generated-code comparison of two versions of a file under csrc/kernels/ (written for ddh.hip), kernel by kernel, without a GPU:
  python profiles/tools/ddh_codegen_compare.py OLD.hip NEW.hip [--keep DIR] [--flags-of NAME.hip]
Compiles both to gfx950 assembly with build.py's flags for NEW's file name (--flags-of: for this file name instead, when
neither copy carries the name it has in the tree) and prints, for every __global__ instantiation, the
registers, scratch, LDS, the instruction count, whether the mnemonic histogram is the same and a sequence diff (mnemonics
left unmatched by difflib's longest-matching-blocks alignment, removed + added: 0 = the same instructions in the same order,
registers aside; a non-zero figure is an upper bound on what moved, not a minimal edit distance), and the same three for
the blocks that lie inside loops (the time stepping, where these kernels spend their time), and whether the instruction text, operands
included (block labels renumbered per kernel), is the same line for line.  A new kernel with more than one innermost loop
(the element-lane march with the sources in the first pass only has two time loops) gets a line per innermost loop, with what it
holds and what of ds_*, scratch_* and v_readlane / v_writelane is in it, and where a loop has LDS accesses, at which instruction
they, the s_waitcnt and the DPP instructions stand.  A kernel that differs is to be
timed against the old build; same histogram does not mean same speed for kernels tuned on issue order."""
import collections
import difflib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from cuddhelmholtz_amd import build as B  # noqa: E402

# kernels whose symbol changed, per file: demangled name (without the argument list) in OLD -> in NEW
RENAMED = {"ddh.hip": {"ddh_mfma_kernel<float>": "ddh_mfma_kernel<float, false, false>", "ddh_mfma_kernel<double>": "ddh_mfma_kernel<double, false, false>",
                       # ddh_block_kernel got its launch bound as a fourth template argument; 256 is the bound it had
                       **{f"ddh_block_kernel<{real}, {nb}, {csr}>": f"ddh_block_kernel<{real}, {nb}, {csr}, 256>"
                          for real in ("float", "double") for nb in range(2, 11) for csr in ("false", "true")},
                       # ddh_element_lane_kernel got PAIRED as a fourth template argument (false is the chains it had), then NB as
                       # the first, when ddh_element_lane5_kernel became its NB = 5 instantiations
                       **{f"ddh_element_lane_kernel<{f}, {h}, {l}{g}>": f"ddh_element_lane_kernel<4, {f}, {h}, {l}, false{g}>"
                          for f in ("false", "true") for h in ("false", "true") for l in ("false", "true") for g in ("", ", TimeGrids<float> ")},
                       **{f"ddh_element_lane_kernel<{f}, {h}, {l}, {p}{g}>": f"ddh_element_lane_kernel<4, {f}, {h}, {l}, {p}{g}>"
                          for f in ("false", "true") for h in ("false", "true") for l in ("false", "true") for p in ("false", "true")
                          for g in ("", ", TimeGrids<float> ")},
                       **{f"ddh_element_lane5_kernel<{f}, {h}, {l}{g}>": f"ddh_element_lane_kernel<5, {f}, {h}, {l}, false{g}>"
                          for f in ("false", "true") for h in ("false", "true") for l in ("false", "true") for g in ("", ", TimeGrids<float> ")}}}
# the same for names that changed by a rule, per file: (pattern, replacement) pairs applied to OLD's demangled name give NEW's.
# wave_stages.hpp became a template on the scalar (round 26, fp32 lattice sweeps): Rk2A is now Rk2AT<double>
_STAGE_RULES = ((r"\b(?:cuddh_k::wave::)?(Begin|Rk2A|Rk2B|Rk4First|Rk4Mid|Rk4Last)\b(?!T)", r"cuddh_k::wave::\1T<double>"),)
# ddh_element_lane_kernel got ONCE as its sixth template argument, before the grids (false is the march it had)
_ONCE_RULE = ((r"(ddh_element_lane_kernel<\d, \w+, \w+, \w+, \w+)((?:, TimeGrids<\w+> ?)?>)$", r"\1, false\2"),)
# and SCALED as its seventh (false is the march it had); applied after _ONCE_RULE, so a name from before either gets both
_SCALED_RULE = ((r"(ddh_element_lane_kernel<\d, \w+, \w+, \w+, \w+, \w+)((?:, TimeGrids<\w+> ?)?>)$", r"\1, false\2"),)
# and CARRIED as its eighth (false is the head it had); applied last, so a name from before any of the three gets all
_CARRIED_RULE = ((r"(ddh_element_lane_kernel<\d, \w+, \w+, \w+, \w+, \w+, \w+)((?:, TimeGrids<\w+> ?)?>)$", r"\1, false\2"),)
# and FETCHED as its ninth (false is the DPP assembly it had); applied last, so a name from before any of the four gets all
_FETCHED_RULE = ((r"(ddh_element_lane_kernel<\d, \w+, \w+, \w+, \w+, \w+, \w+, \w+)((?:, TimeGrids<\w+> ?)?>)$", r"\1, false\2"),)
RENAMED_BY_RULE = {"waveholtz.hip": _STAGE_RULES, "wave_lattice.hip": _STAGE_RULES, "ddh.hip": _ONCE_RULE + _SCALED_RULE + _CARRIED_RULE + _FETCHED_RULE}
# instantiations that are another one plus (or with another) template argument, per file: (pattern, replacement) pairs applied to the
# demangled name give the base.
# A new kernel with a base in NEW is printed against it (registers, scratch, loop contents, vector instructions in the loops).
DERIVED = {"ddh.hip": ((r", Rk4Scheme ?(?=>)|, TimeGrids<\w+> ?(?=>)", ""),
                       # the paired chains (PAIRED = true, one grid only) against the pinned ones
                       (r"(ddh_element_lane_kernel<\w+, \w+, \w+, \w+), true, false, false, false, false>", r"\1, false, false, false, false, false>"),
                       # the sources in the first pass only (ONCE = true, beside the paired chains only) against every pass
                       (r"(ddh_element_lane_kernel<\w+, \w+, \w+, \w+, true), true, false, false, false>", r"\1, false, false, false, false>"),
                       # the scaled march (SCALED = true, beside ONCE only) against the march it is derived from
                       (r"(ddh_element_lane_kernel<\w+, \w+, \w+, \w+, true, true), true, false, false>", r"\1, false, false, false>"),
                       # the carried head (CARRIED = true, beside SCALED only) against the scaled march
                       (r"(ddh_element_lane_kernel<\w+, \w+, \w+, \w+, true, true, true), true, false>", r"\1, false, false>"),
                       # the assembly over the LDS pipe (FETCHED = true, beside CARRIED only) against the DPP assembly
                       (r"(ddh_element_lane_kernel<\w+, \w+, \w+, \w+, true, true, true, true), true>", r"\1, false>"))}
INNER = {}  # (assembly file, kernel) -> its innermost loops
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(src: Path, out: Path, flags_of: str):
    cmd = [B.hipcc(), *B.COMMON, *[f"-I{p}" for p in B.INCLUDES], *B.HIP_FLAGS, *B.EXTRA_FLAGS.get(flags_of, []), "--cuda-device-only", "-S",
           str(src), "-o", str(out)]
    subprocess.run(cmd, check=True)
    text = out.read_text()
    found = {}
    # the metadata holds one list item per kernel under amdhsa.kernels (items start with "  - ", their fields with "    ")
    for entry in re.split(r"\n  - (?=\.)", text.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0])[1:]:
        sym = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M).group(1)
        meta = {f: int(re.search(rf"^\s*{re.escape(f)}:\s+(\d+)", entry, re.M).group(1)) for f in FIELDS}
        body = text.split(f"\n{sym}:", 1)[1].split(".Lfunc_end", 1)[0]
        ops, loop_ops, lines, in_loop = [], [], [], False
        inner, inner_header, in_inner = [], None, False  # the innermost loops, block by block: a list of mnemonics each
        for ln in body.splitlines():
            if ln.startswith((".LBB", "; %bb")):  # the compiler marks every block of a loop in the label's comment
                in_loop = "Loop" in ln
                in_inner = inner_header is not None and f"in Loop: Header={inner_header} " in ln
                if "This Inner Loop Header" in ln:
                    inner_header, in_inner = ln.split(":")[0].removeprefix(".L"), True
                    inner.append([])
                label = ln.split(":")[0].removeprefix(".L")
            elif ln.lstrip().startswith(";") and "This Inner Loop Header" in ln:  # the comment goes on below the label
                inner_header, in_inner = label, True
                inner.append([])
            elif ln.startswith("\t") and ln[1:2] not in ("", ".", ";"):
                ops.append(ln.split()[0])
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(ln.split(";")[0].split())))
                if in_loop:
                    loop_ops.append(ops[-1])
                if in_inner:
                    inner[-1].append(ops[-1])
        name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        name = name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
        found[name] = (meta, ops, loop_ops, lines)
        INNER[(str(out), name)] = inner
    return found


def main():
    keep = Path(sys.argv[sys.argv.index("--keep") + 1]) if "--keep" in sys.argv else Path(tempfile.mkdtemp())
    keep.mkdir(parents=True, exist_ok=True)
    flags_of = sys.argv[sys.argv.index("--flags-of") + 1] if "--flags-of" in sys.argv else Path(sys.argv[2]).name
    renamed = RENAMED.get(flags_of, {})
    old, new = kernels(Path(sys.argv[1]), keep / "old.s", flags_of), kernels(Path(sys.argv[2]), keep / "new.s", flags_of)
    print(f"{len(old)} kernels before, {len(new)} after")
    print("kernel | vgpr sgpr scratch lds before -> after | instructions before -> after | histogram | sequence diff | inside loops")
    same = same_text = 0
    old_in_new = {}  # NEW's version of the kernels OLD has
    for name, (m0, o0, l0, t0) in old.items():
        succ = name if name in new else renamed.get(name, name)
        for pattern, repl in RENAMED_BY_RULE.get(flags_of, ()):
            if succ not in new:
                succ = re.sub(pattern, repl, succ)
        if succ not in new:
            print(f"{name} | MISSING after")
            continue
        m1, o1, l1, t1 = new.pop(succ)
        old_in_new[succ] = (m1, o1, l1)
        hist = collections.Counter(o0) == collections.Counter(o1)
        # mnemonics removed + added by a longest-matching-blocks alignment (autojunk off: a few dozen distinct values repeat
        # thousands of times); not a minimal edit distance, but 0 means identical and small means a few moved instructions
        moved = lambda a, b: len(a) + len(b) - 2 * sum(m.size for m in difflib.SequenceMatcher(None, a, b, autojunk=False).get_matching_blocks())  # noqa: E731
        diff = moved(o0, o1)
        c0, c1 = collections.Counter(l0), collections.Counter(l1)
        loops = f"{len(l0)} -> {len(l1)}, sequence diff {moved(l0, l1)}, " + ("same histogram" if c0 == c1 else
                "DIFFERS " + " ".join(f"{k}:{c0[k]}->{c1[k]}" for k in sorted(set(c0) | set(c1)) if c0[k] != c1[k]))
        regs = lambda m: " ".join(str(m[f]) for f in FIELDS)  # noqa: E731
        same += m0 == m1 and hist and diff == 0
        same_text += m0 == m1 and t0 == t1
        label = name if succ == name else f"{name} => {succ}"
        print(f"{label} | {regs(m0)} -> {regs(m1)} | {len(o0)} -> {len(o1)} | {'same' if hist else 'DIFFERS'} | {diff} | {loops} | text {'same' if t0 == t1 else 'DIFFERS'}")
    all_new = {**{renamed.get(k, k): v for k, v in old_in_new.items()}, **new}
    derived = DERIVED.get(flags_of)
    valu = lambda c: sum(v for k, v in c.items() if k.startswith("v_"))  # noqa: E731
    for name, (m1, o1, l1, _) in new.items():  # a kernel the old file does not have: its registers and what its loops hold
        c1 = collections.Counter(l1)
        base = name
        for pattern, repl in derived or ():
            base = re.sub(pattern, repl, base)
        if base != name and base in all_new:
            m0, _, l0 = all_new[base][:3]
            c0 = collections.Counter(l0)
            regs = lambda m: " ".join(str(m[f]) for f in FIELDS)  # noqa: E731
            print(f"{name} | NEW after, against {base} | {regs(m0)} -> {regs(m1)} | inside loops {len(l0)} -> {len(l1)}, vector instructions "
                  f"{valu(c0)} -> {valu(c1)}" + ("" if c0 == c1 else ", " + " ".join(f"{k}:{c0[k]}->{c1[k]}" for k in sorted(set(c0) | set(c1)) if c0[k] != c1[k])))
            loops1, loops0 = INNER[(str(keep / "new.s"), name)], INNER[(str(keep / "new.s"), base)]
            if len(loops1) > 1:  # every innermost loop by itself, against the base's (first) one
                b = collections.Counter(loops0[0]) if loops0 else collections.Counter()
                for i, lp in enumerate(loops1):
                    c = collections.Counter(lp)
                    barred = sum(v for k, v in c.items() if k.startswith(("ds_", "scratch_", "v_readlane", "v_writelane")))
                    print(f"    innermost loop {i + 1} of {len(loops1)}: {len(lp)} instructions, vector {valu(c)} (the base's loop {valu(b)}), "
                          f"ds_* / scratch_* / v_readlane / v_writelane {barred}, against the base's: "
                          + (" ".join(f"{k}:{b[k]}->{c[k]}" for k in sorted(set(b) | set(c)) if b[k] != c[k]) or "same histogram"))
                    if any(k.startswith("ds_") for k in lp):  # where the LDS accesses stand, and the waits behind them
                        at = lambda pre: " ".join(f"{i}:{k}" if pre == "ds_" else str(i) for i, k in enumerate(lp) if k.startswith(pre))  # noqa: E731
                        print(f"        ds_* at (instruction of {len(lp)}) {at('ds_')}; s_waitcnt at {at('s_waitcnt')}; DPP at "
                              f"{' '.join(str(i) for i, k in enumerate(lp) if k.endswith('_dpp'))}")
            continue
        print(f"{name} | NEW after | {' '.join(str(m1[f]) for f in FIELDS)} | {len(o1)} instructions, {len(l1)} inside loops: "
              + " ".join(f"{k}:{c1[k]}" for k in sorted(c1)))
    print(f"{same} of {len(old)} kernels: same registers, same mnemonic sequence; {same_text} of {len(old)}: same registers and the same instruction text, "
          "operands included")


if __name__ == "__main__":
    main()
