"""Development aid: is the device code of two source trees the same, instruction for instruction?  (Minutes, no GPU.)

For a change that must not move an instruction -- a split of a header, an extraction inside a kernel -- this replaces an A/B benchmark,
which resolves such a move only at the 1 % level.  Each tree's twl_align.hip is compiled device-only to gfx950 assembly with the product's HIP_FLAGS
(__graft_entry__.py, without -shared / -fPIC: no library is linked); the listing is cut per kernel symbol (entry label to the end of the kernel descriptor, so
registers, scratch and LDS are compared with the text), comments and the per-compilation __hip_cuid_* symbol are dropped, local labels are renumbered in order of
appearance, and the texts are compared.  Whatever lies outside the kernels (device variables, metadata) is compared as one more entry.  Text only: no instruction
is looked for.

    git worktree add /tmp/twl_parent HEAD~1            (or: git archive HEAD~1 | tar -x -C /tmp/twl_parent)
    python tools/isa_compare.py /tmp/twl_parent .      ->  one line per kernel: instructions, same / DIFFER; a total; exit status 1 when anything differs

An argument that is a file is taken as a listing made earlier (--keep DIR leaves a.s and b.s there); extra compiler flags go behind `--`."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIP_FLAGS, HIPCC  # noqa: E402

LOCAL = re.compile(r"\.L[A-Za-z_$.]*\d+(?:_\d+)?")


def listing(tree, out, extra):
    """assembly of tree/twilight_amd/csrc/twl_align.hip, device side only"""
    if os.path.isfile(tree):
        return open(tree).read()
    csrc = os.path.join(os.path.abspath(tree), "twilight_amd", "csrc")
    flags = [f for f in HIP_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([HIPCC] + flags + list(extra) + ["-S", "--cuda-device-only", "-o", out, "twl_align.hip"], cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree}: the compiler failed\n{r.stderr[-3000:]}")
    return open(out).read()


def normalise(lines):
    """comments, blank lines and __hip_cuid_* lines out; local labels renumbered in order of appearance"""
    names, out = {}, []
    for l in lines:
        l = l.split(";", 1)[0].rstrip()
        if not l.strip() or "__hip_cuid_" in l:
            continue
        out.append(LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), l))
    return out


def cut(text):
    """{kernel symbol: its lines from the entry label to .end_amdhsa_kernel}, and the lines outside every kernel"""
    lines = text.split("\n")
    kernels = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    want, parts, rest, cur = set(kernels), {}, [], None
    for l in lines:
        if cur is None and l[:1] == "_" and l.split(":", 1)[0] in want:      # (the entry label: "<symbol>:   ; @<symbol>")
            cur = l.split(":", 1)[0]
            parts[cur] = []
        (parts[cur] if cur else rest).append(l)
        if cur and l.strip() == ".end_amdhsa_kernel":
            cur = None
    # (what the assembler names a kernel in front of its entry label -- .globl, .type, .p2align -- stays in `rest`, with the kernel's name in it)
    return {k: normalise(v) for k, v in parts.items()}, normalise(rest)


def instructions(body):
    n = 0
    for l in body:
        if l.startswith("\t.section"):
            break
        n += 1 if re.match(r"\t[a-z]", l) else 0
    return n


def main(argv):
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    keep = None
    if "--keep" in argv:
        keep = argv[argv.index("--keep") + 1]
        del argv[argv.index("--keep"):argv.index("--keep") + 2]
    if len(argv) != 2:
        sys.exit(__doc__)
    d = keep or tempfile.mkdtemp(prefix="twl_isa_")
    os.makedirs(d, exist_ok=True)
    with ThreadPoolExecutor(2) as ex:
        ta, tb = ex.map(lambda p: listing(p[0], os.path.join(d, p[1]), extra), [(argv[0], "a.s"), (argv[1], "b.s")])
    (ka, ra), (kb, rb) = cut(ta), cut(tb)
    demangle = dict(zip(list(ka) + list(kb), subprocess.run(["c++filt"], input="\n".join(list(ka) + list(kb)), capture_output=True, text=True).stdout.split("\n")))
    differ = 0
    print(f"# A = {argv[0]}   B = {argv[1]}   flags: {' '.join(f for f in HIP_FLAGS if f not in ('-shared', '-fPIC'))} {' '.join(extra)}")
    print("# instructions in A / in B, verdict, kernel")
    for k in list(ka) + [k for k in kb if k not in ka]:
        a, b = ka.get(k), kb.get(k)
        verdict = "same" if a == b else ("DIFFER" if a is not None and b is not None else ("only in A" if b is None else "only in B"))
        differ += verdict != "same"
        print(f"{instructions(a) if a is not None else '-':>7} {instructions(b) if b is not None else '-':>7}  {verdict:9s} {demangle.get(k, k)}")
    verdict = "same" if ra == rb else "DIFFER"
    differ += verdict != "same"
    print(f"{len(ra):>7} {len(rb):>7}  {verdict:9s} (lines outside the kernels: symbols, device variables, metadata)")
    print(f"total: {len(ka)} kernels in A, {len(kb)} in B, {sum(instructions(v) for v in ka.values())} / {sum(instructions(v) for v in kb.values())} instructions, {differ} differing")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
