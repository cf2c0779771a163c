"""Source-level ledger of everything in csrc that touches the null stream ("Stream contract").

Every launch of the library goes to cuddh::stream().  What does not -- a blocking hipMemcpy / hipMemset, a
hipDeviceSynchronize, an *Async call or a kernel launch with a literal null stream -- is correct only for a reason that lives
somewhere else in the code: a stream sync in the caller, a buffer that no stream has touched yet.  LEDGER lists every such call
with that reason, keyed by (file, enclosing function, call).  The test fails when the tree holds a call the ledger does not
list and when the ledger lists one the tree no longer has, so a new null-stream call cannot arrive without a written reason.
tests/test_gpu_stream_order.py is the run-time half: the same entry points on a non-blocking side stream with delayed inputs.

Calls are found by parsing to the matching parenthesis (launches span lines), with comments and string literals blanked.
"""
import functools
import re
from collections import Counter
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "cuddhelmholtz_amd" / "csrc"
SCANNED = ("kernels", "src", "include")
SUFFIXES = (".hip", ".cpp", ".hpp", ".h")

# always on the null stream, and blocking
BLOCKING = ("hipMemcpy", "hipMemset", "hipDeviceSynchronize")
# on the null stream when the stream argument (at this index) is a literal null
STREAMED = {"hipMemsetAsync": 3, "hipMemcpyAsync": 4, "hipStreamSynchronize": 0, "hipLaunchKernelGGL": 4}
NULL_STREAM = re.compile(r"^(?:\(\s*hipStream_t\s*\)\s*)?(?:nullptr|NULL|0|hipStreamDefault|hipStream_t\s*\{\s*\}|hipStream_t\s*\(\s*(?:0|nullptr)?\s*\))$")
CALL = re.compile(r"\b(" + "|".join(BLOCKING + tuple(STREAMED)) + r")\s*\(")
NOT_A_FUNCTION = {"if", "for", "while", "switch", "catch", "return", "sizeof", "decltype", "alignas", "noexcept", "requires", "static_assert"}


def blank_comments_and_strings(text: str) -> str:
    """The text with every comment, string and character literal replaced by spaces: offsets and line numbers are kept."""
    out = list(text)
    i, n = 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
        elif c == '"' and text.startswith('R"', i - 1) and i > 0:
            d = text.index("(", i)
            close = ")" + text[i + 1:d] + '"'
            j = text.index(close, d) + len(close)
        elif c in "\"'":
            if c == "'" and i > 0 and text[i - 1].isalnum():  # a digit separator, 1'000
                i += 1
                continue
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            j += 1
        else:
            i += 1
            continue
        for k in range(i, min(j, n)):
            if out[k] != "\n":
                out[k] = " "
        i = j
    return "".join(out)


def matching_paren(code: str, open_at: int) -> int:
    """Index of the parenthesis that closes the one at open_at (code: comments and strings already blanked)."""
    depth = 0
    for i in range(open_at, len(code)):
        if code[i] == "(":
            depth += 1
        elif code[i] == ")":
            depth -= 1
            if depth == 0:
                return i
    raise ValueError(f"unbalanced parenthesis at offset {open_at}")


def split_args(inner: str) -> list:
    """The top-level arguments of a call, whitespace collapsed.  Commas inside (), [] and {} do not split; a template argument
    list with a comma has to be parenthesised to be a macro argument at all, so <> needs no counting."""
    args, depth, start = [], 0, 0
    for i, c in enumerate(inner):
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
        elif c == "," and depth == 0:
            args.append(inner[start:i])
            start = i + 1
    args.append(inner[start:])
    args = [" ".join(a.split()) for a in args]
    return [] if args == [""] else args


def function_scopes(code: str) -> list:
    """(open, close, name) of every brace block that is a function body: a '{' that follows the ')' of a parameter list, with
    qualifiers (const, noexcept, override, a trailing return type) between them, whose '(' follows an identifier that is no
    control keyword.  Lambdas ('](') and control statements are no functions: what they hold belongs to the function around."""
    scopes, stack = [], []
    for i, c in enumerate(code):
        if c == "{":
            stack.append((i, _function_name(code, i)))
        elif c == "}" and stack:
            o, name = stack.pop()
            if name:
                scopes.append((o, i, name))
    return scopes


_QUALIFIERS = re.compile(r"(?:\s|\bconst\b|\bnoexcept\b|\boverride\b|\bfinal\b|\bmutable\b|->\s*[\w:<>,\s\*&]+?)*")
_NAME = re.compile(r"([A-Za-z_~][\w:~]*)\s*(?:<[^;{}()]*>)?\s*$")


def _function_name(code: str, brace: int) -> str:
    close = code.rfind(")", max(0, brace - 120), brace)
    if close < 0 or not _QUALIFIERS.fullmatch(code, close + 1, brace):
        return ""
    depth = 0
    for i in range(close, -1, -1):  # back to the '(' of the parameter list
        if code[i] == ")":
            depth += 1
        elif code[i] == "(":
            depth -= 1
            if depth == 0:
                break
    else:
        return ""
    m = _NAME.search(code, max(0, i - 200), i)
    if not m or m.group(1).split("::")[-1] in NOT_A_FUNCTION:
        return ""
    return m.group(1)


def describe(name: str, args: list) -> str:
    """What identifies a call in the ledger: its name and the arguments that say what it touches."""
    if name == "hipLaunchKernelGGL":
        return f"launch {args[0].strip('() ')}" if args else "launch"
    if name in ("hipMemcpy", "hipMemcpyAsync"):
        return f"{name}({', '.join(args[:2])})"
    if name in ("hipMemset", "hipMemsetAsync"):
        return f"{name}({', '.join(args[:1])})"
    return f"{name}({', '.join(args[:1])})"


@functools.lru_cache(maxsize=None)
def scan_text(text: str, rel: str) -> tuple:
    """[(file, function, call, line)] of every null-stream call in one file's text."""
    code = blank_comments_and_strings(text)
    scopes = function_scopes(code)
    found = []
    for m in CALL.finditer(code):
        name = m.group(1)
        open_at = m.end() - 1
        args = split_args(code[open_at + 1:matching_paren(code, open_at)])
        if name in STREAMED:
            at = STREAMED[name]
            if len(args) <= at or not NULL_STREAM.match(args[at]):
                continue
        around = [s for s in scopes if s[0] < m.start() < s[1]]
        function = min(around, key=lambda s: s[0])[2] if around else "<file scope>"  # the outermost: local structs and lambdas belong to it
        found.append((rel, function, describe(name, args), code.count("\n", 0, m.start()) + 1))
    return tuple(found)


def scan_tree(root: Path = CSRC) -> list:
    found = []
    for sub in SCANNED:
        for path in sorted((root / sub).rglob("*")):
            if path.suffix in SUFFIXES:
                found += scan_text(path.read_text(), f"{sub}/{path.relative_to(root / sub).as_posix()}")
    return found


_DDH_PLAN = ("DDHCore::ensure_plan syncs stream() after the last table upload and geom_setup (ddh.cpp, 'DDH table upload'), right before "
             "plan creation: ")
_HELM_PLAN = ("the metric arrays are complete: every operator's setup() ends in a sync of stream() (operators.cpp), and plan creation "
              "runs after the constructors: ")

# (file, enclosing function, call) -> (occurrences, what orders it against stream())
LEDGER = {
    ("kernels/ddh.hip", "device_flag_check", "hipMemset(flag)"):
        (1, "a flag allocated two lines above, which no stream has touched; the check kernel follows on the same null stream"),
    ("kernels/ddh.hip", "device_flag_check", "hipMemcpy(bad, flag)"):
        (1, "blocking read on the null stream, behind the check kernel launched on the null stream one line above"),
    ("kernels/ddh.hip", "check_uniform_geometry", "launch ddh_uniform_check_kernel<Real>"):
        (1, _DDH_PLAN + "d.G is complete; the flag read that follows is on the null stream too"),
    ("kernels/ddh.hip", "establish_facts", "launch ddh_wave_check_kernel<NB, NEL>"):
        (1, _DDH_PLAN + "d.s_dof and d.sI are complete; the flag read that follows is on the null stream too"),
    ("kernels/ddh.hip", "establish_facts", "launch ddh_interior_check_kernel"):
        (1, _DDH_PLAN + "d.s_fdof and d.sI are complete; the flag read that follows is on the null stream too"),
    ("kernels/ddh.hip", "build_dense_element_matrix", "hipMemcpy(hD, d.D)"):
        (1, _DDH_PLAN + "d.D is complete and never written again"),
    ("kernels/ddh.hip", "build_dense_element_matrix", "hipMemcpy(hG, d.G)"):
        (1, _DDH_PLAN + "d.G is complete and never written again"),
    ("kernels/ddh.hip", "build_dense_element_matrix", "hipMemcpy(dA, hA)"):
        (1, "blocking upload from pageable memory into a buffer allocated one line above; done when it returns, before any launch can read it"),
    ("kernels/ddh.hip", "download_element", "hipMemcpy(hD, d.D)"):
        (1, _DDH_PLAN + "d.D is complete and never written again"),
    ("kernels/ddh.hip", "download_element", "hipMemcpy(hG, d.G)"):
        (1, _DDH_PLAN + "d.G is complete and never written again"),
    ("kernels/ddh.hip", "upload_table", "hipMemcpy(*dst, h)"):
        (1, "blocking upload from pageable memory into a buffer allocated one line above; done when it returns, before any launch can read it"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_create_general", "hipMemcpy(sI.data(), desc->sI)"):
        (1, _DDH_PLAN + "desc->sI is complete and never written again"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_create_general", "hipMemcpy(s_dof.data(), desc->s_dof)"):
        (1, _DDH_PLAN + "desc->s_dof is complete and never written again"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_create_general", "hipMemcpy(s_fdof.data(), desc->s_fdof)"):
        (1, _DDH_PLAN + "desc->s_fdof is complete and never written again"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_create_general", "hipMemcpy(p->csr_off, off.data())"):
        (1, "blocking upload from pageable memory into a fresh allocation of the plan; done when it returns, before any launch can read it"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_create_general", "hipMemcpy(p->csr_src, src.data())"):
        (1, "blocking upload from pageable memory into a fresh allocation of the plan; done when it returns, before any launch can read it"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_set_time_grids", "hipMemcpy(grid_of.data(), d_grid_of)"):
        (1, _DDH_PLAN + "grid_of was uploaded before that sync and is never written again"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_set_time_grids", "hipMemcpy(d_grids, h.data())"):
        (1, "blocking upload from pageable memory into a fresh allocation; done when it returns, and the plan takes the pointer only afterwards"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_set_time_grids", "hipMemcpy(d_order, order.data())"):
        (1, "blocking upload from pageable memory into a fresh allocation; done when it returns, and the plan takes the pointer only afterwards"),
    ("kernels/ddh.hip", "cuddh_hip_ddh_plan_set_time_grids", "hipMemcpy(d_index, index.data())"):
        (1, "blocking upload from pageable memory into a fresh allocation; done when it returns, and the plan takes the pointer only afterwards"),
    ("kernels/helmholtz_fused.hip", "upload", "hipMemcpy(*dst, v.data())"):
        (1, "blocking upload from pageable memory into a buffer allocated one line above; done when it returns, before any launch can read it"),
    ("kernels/helmholtz_fused.hip", "uniform_block", "hipMemcpy(first.data(), d_src)"):
        (1, _HELM_PLAN + "element 0's block of the metric array is final"),
    ("kernels/helmholtz_fused.hip", "uniform_block", "hipMemset(flag)"):
        (1, "a flag allocated two lines above, which no stream has touched; the kernel that raises it follows on the same null stream"),
    ("kernels/helmholtz_fused.hip", "uniform_block", "launch uniform_metric_kernel"):
        (1, _HELM_PLAN + "it reads the metric array alone, and the flag read that follows is on the null stream too"),
    ("kernels/helmholtz_fused.hip", "uniform_block", "hipMemcpy(&differs, flag)"):
        (1, "blocking read on the null stream, behind the kernel launched on the null stream one line above"),
    ("kernels/helmholtz_fused.hip", "build_plan", "hipMemset(p->stamps)"):
        (1, "a fresh allocation of the plan; the hipDeviceSynchronize that ends plan creation completes it before any apply"),
    ("kernels/helmholtz_fused.hip", "build_plan", "hipMemset(d_zero)"):
        (1, "a fresh scratch array, read only by the repack kernels that follow on the same null stream"),
    ("kernels/helmholtz_fused.hip", "build_plan", "launch repack_mfma_kernel"):
        (2, _HELM_PLAN + "the kernels read them into fresh arrays of the plan, complete at the hipDeviceSynchronize below"),
    ("kernels/helmholtz_fused.hip", "build_plan", "launch repack_kernel"):
        (2, _HELM_PLAN + "the kernels read them into fresh arrays of the plan, complete at the hipDeviceSynchronize below"),
    ("kernels/helmholtz_fused.hip", "build_plan", "hipDeviceSynchronize()"):
        (1, "set-up only, once per plan: completes the null-stream repack kernels before the scratch is freed and stream() applies the plan"),
    ("kernels/helmholtz_fused.hip", "cuddh_hip_helmholtz_plan_read_stamps", "hipMemcpy(h_out, p->stamps)"):
        (1, "a diagnostic of the C ABI (CUDDH_HELM_STAMPS), outside every apply: its callers (profiles/tools/*_stamps.py) synchronise the device first"),
    ("kernels/runtime.hip", "cuddh_hip_malloc_zeroed", "hipMemsetAsync(*ptr)"):
        (1, "a fresh allocation no stream has touched; the null-stream sync on the next line completes the fill before the pointer is returned"),
    ("kernels/runtime.hip", "cuddh_hip_malloc_zeroed", "hipStreamSynchronize(nullptr)"):
        (1, "completes the fill above; allocation only (HostDeviceArray, the GMRES basis, the reduction workspace), never inside an apply"),
    ("kernels/runtime.hip", "cuddh_hip_copy_h2d", "hipMemcpy(dst, h_src)"):
        (1, "C ABI for callers without a stream, unused by the library itself, which copies with cuddh_hip_copy_h2d_on(stream())"),
    ("kernels/runtime.hip", "cuddh_hip_copy_d2h", "hipMemcpy(h_dst, src)"):
        (1, "C ABI for callers without a stream, unused by the library itself, which copies with cuddh_hip_copy_d2h_on(stream())"),
    ("kernels/runtime.hip", "cuddh_hip_device_sync", "hipDeviceSynchronize()"):
        (1, "C ABI: the device-wide sync itself, exported for hosts and examples; the library never calls it on an apply path"),
}


def check(found: list, ledger: dict) -> list:
    """What is wrong between the occurrences found and the ledger, one line each (empty: they agree)."""
    have = Counter((f, fn, call) for f, fn, call, _ in found)
    lines = {}
    for f, fn, call, line in found:
        lines.setdefault((f, fn, call), []).append(line)
    problems = []
    for key, count in sorted(have.items()):
        want = ledger.get(key)
        if want is None:
            problems.append(f"not in the ledger: {key[0]}:{lines[key][0]} in {key[1]}: {key[2]}")
        elif want[0] != count:
            problems.append(f"ledger lists {want[0]}, tree has {count} (lines {lines[key]}): {key}")
    for key in sorted(set(ledger) - set(have)):
        problems.append(f"ledger lists a call the tree no longer has: {key}")
    for key, (count, reason) in ledger.items():
        if count < 1 or len(reason.split()) < 4:
            problems.append(f"ledger entry without a count or a reason: {key}")
    return problems


def test_every_null_stream_call_is_in_the_ledger():
    found = scan_tree()
    assert len(found) >= 30, "the scanner found next to nothing: it is broken, not the tree clean"
    problems = check(found, LEDGER)
    assert not problems, "\n".join(problems)


def test_scanner_reads_the_files_the_library_is_built_from():
    files = {f for f, _, _, _ in scan_tree()}
    assert {"kernels/ddh.hip", "kernels/helmholtz_fused.hip", "kernels/runtime.hip"} <= files
    text = (CSRC / "kernels" / "ddh.hip").read_text()
    assert "hipLaunchKernelGGL" in text and "as_stream(stream)" in text  # launches on a stream exist and are not reported
    assert all(f == "kernels/ddh.hip" for f, _, _, _ in scan_text(text, "kernels/ddh.hip"))


_ADDED = """
    int stray_helper(const cuddh_ddh_desc &d, int *flag)
    {
        hipLaunchKernelGGL((ddh_wave_check_kernel<4, 4>),
                           dim3(d.n_domains), dim3(256), 0,
                           nullptr, // the stream
                           d.n_domains, d.s_dof, d.sI, flag);
        return 0;
    }
"""


def test_an_added_null_stream_launch_fails(tmp_path):
    """a scratch copy of ddh.hip with one multi-line launch on nullptr: found, named, refused"""
    src = (CSRC / "kernels" / "ddh.hip").read_text()
    at = src.index("    template <typename Launch>\n    int device_flag_check")
    scratch = tmp_path / "ddh.hip"
    scratch.write_text(src[:at] + _ADDED + src[at:])
    found = [o for o in scan_tree() if o[0] != "kernels/ddh.hip"] + list(scan_text(scratch.read_text(), "kernels/ddh.hip"))
    problems = check(found, LEDGER)
    assert len(problems) == 1 and "stray_helper" in problems[0] and "launch ddh_wave_check_kernel<4, 4>" in problems[0], problems


def test_a_second_copy_of_a_listed_call_fails(tmp_path):
    """the ledger counts: one more blocking copy inside a function that already has one is refused"""
    src = (CSRC / "kernels" / "ddh.hip").read_text()
    line = "        hipError_t e = hipMemcpy(hD, d.D, sizeof hD, hipMemcpyDeviceToHost);\n"
    assert src.count(line) == 2
    at = src.index(line)
    text = src[:at] + "        (void)hipMemcpy(hD, d.D, sizeof hD, hipMemcpyDeviceToHost);\n" + src[at:]
    found = [o for o in scan_tree() if o[0] != "kernels/ddh.hip"] + list(scan_text(text, "kernels/ddh.hip"))
    problems = check(found, LEDGER)
    assert len(problems) == 1 and "ledger lists 1, tree has 2" in problems[0], problems


def test_a_listed_call_that_left_the_tree_fails():
    """the tree without runtime.hip's zero fill, and the ledger without one entry the tree still has: both refused"""
    src = (CSRC / "kernels" / "runtime.hip").read_text()
    line = "        e = hipMemsetAsync(*ptr, 0, bytes, nullptr);\n"
    assert src.count(line) == 1
    found = [o for o in scan_tree() if o[0] != "kernels/runtime.hip"] + list(scan_text(src.replace(line, ""), "kernels/runtime.hip"))
    problems = check(found, LEDGER)
    assert len(problems) == 1 and "no longer has" in problems[0] and "hipMemsetAsync(*ptr)" in problems[0], problems
    key = ("kernels/ddh.hip", "device_flag_check", "hipMemset(flag)")
    problems = check(scan_tree(), {k: v for k, v in LEDGER.items() if k != key})
    assert len(problems) == 1 and "not in the ledger" in problems[0] and "device_flag_check" in problems[0], problems


def test_comments_strings_and_streamed_calls_are_not_reported():
    text = '''
    namespace k {
    // hipMemcpy(a, b, n, hipMemcpyDeviceToHost); in a comment
    /* hipDeviceSynchronize(); in another */
    const char *doc = "hipMemset(p, 0, n) in a string";
    struct Plan { int n; };
    template <typename T>
    int good(T *p, size_t n, hipStream_t st) noexcept
    {
        hipError_t e = hipMemsetAsync(p, 0, n, st);
        hipLaunchKernelGGL((kern<T, 4>), dim3(g(n, 256)), dim3(256), 0, as_stream(st), p, nullptr, 0);
        if (e == hipSuccess) { e = hipStreamSynchronize(st); }
        return (int)e;
    }
    int bad(double *p, size_t n) const
    {
        auto run = [&](int *flag) { hipLaunchKernelGGL(kern2, dim3(1), dim3(64), 0, 0, p, flag); };
        for (int i = 0; i < 2; ++i) { (void)hipMemcpyAsync(p, p + n, n, hipMemcpyDeviceToDevice, (hipStream_t)0); }
        return (int)hipStreamSynchronize(
            nullptr);
    }
    }
    '''
    got = [(fn, call) for _, fn, call, _ in scan_text(text, "x.hip")]
    assert got == [("bad", "launch kern2"), ("bad", "hipMemcpyAsync(p, p + n)"), ("bad", "hipStreamSynchronize(nullptr)")]


if __name__ == "__main__":
    for f, fn, call, line in scan_tree():
        print(f"{f}:{line}\t{fn}\t{call}")
