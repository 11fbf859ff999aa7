#!/usr/bin/env python3
"""Compare the gfx950 machine code of every kernel symbol in two builds of libgsr_hip.so, symbol by symbol:
    python tools/kernel_disasm_diff.py OLD/libgsr_hip.so NEW/libgsr_hip.so [--pair OLD_TEXT=NEW_TEXT ...] [SYMBOL ...]
(SYMBOL: any part of a mangled name; print the diffs of the differing kernels it matches).  --pair compares the one removed kernel whose demangled name contains OLD_TEXT with the one
kernel of the new build whose demangled name contains NEW_TEXT (several old kernels may pair with the same new one): the way to
follow a rename or a merge without a rule of its own below.  Every kernel that differs is listed with its VGPRs, SGPRs, LDS bytes,
scratch bytes (code-object metadata) and instruction count on both sides.
llvm-objdump disassembles each offload bundle; branch targets, comments and inter-function padding are normalised away.
radix_scatter_kernel gained a trailing template flag CAP (capacity mode, default false), blend_backward_splat_kernel and
geom_backward_kernel one named AUX (include/gsr_aux_grads.h, default false; the blend kernel also two trailing pointer
arguments), and blend_backward_splat_kernel a second one named ABS behind it (include/gsr_densify_stats.h, default false, no new
arguments), and geom_backward_kernel a second one named AA behind AUX (include/gsr_antialias.h, default false) whose two pointer
arguments are a trailing parameter pack, empty when AA is false, so that the classic kernels keep their argument block: an old
instantiation is compared with its flag = false namesake.  preprocess_kernel and camera_partials_kernel were plain functions and
became templates on that same AA flag and pack: a template's mangled name differs throughout, so these two are matched by their
demangled names.  Prints the counts and the symbols that differ, were removed or were added (JSON)."""
import glob, os, re, shutil, subprocess, sys, tempfile, json
OBJ = "/opt/rocm/llvm/bin/llvm-objdump"
META = {}   # (library index, symbol) -> {vgpr, sgpr, lds, scratch}
def kernels(so):
    d = tempfile.mkdtemp()
    s = os.path.join(d, "lib.so"); shutil.copy(so, s)
    subprocess.run([OBJ, "--offloading", s], cwd=d, capture_output=True, check=True)
    out = {}
    for co in sorted(glob.glob(s + ".*gfx950")):
        notes = subprocess.run([OBJ.replace("objdump", "readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            f = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", blk)}
            META[(so, re.search(r"\.name:\s+(\S+)", blk).group(1))] = {"vgpr": f["vgpr_count"], "sgpr": f["sgpr_count"], "lds": f["group_segment_fixed_size"],
                                                                      "scratch": f["private_segment_fixed_size"]}
        txt = subprocess.run([OBJ, "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
            if m:
                cur = m.group(1); out.setdefault(cur, []); continue
            if cur and line.strip():
                l = re.sub(r"<[^>]+>", "<L>", line)           # branch targets
                l = re.sub(r"//.*$", "", l).rstrip()
                if l.strip() == "...":      # inter-function padding
                    continue
                out[cur].append(l)
    shutil.rmtree(d)
    return {k: "\n".join(v) for k, v in out.items()}
pairs = []
while "--pair" in sys.argv:
    i = sys.argv.index("--pair")
    pairs.append(sys.argv[i + 1].split("=", 1))
    del sys.argv[i:i + 2]
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
new_name = {k: k for k in b}   # key in b -> its symbol in the new build (keys move to the old names as kernels are matched)
# kernels that gained a trailing template flag (default false): map each old instantiation to its flag=false name
FLAGGED = ("radix_scatter_kernelI", "blend_backward_splat_kernelI", "geom_backward_kernelI")
renamed = {}
for k in list(a):
    if k not in b and any(f in k for f in FLAGGED):
        i = k.index("EEEv")
        nk = k[:i] + "ELb0" + k[i:]
        if nk not in b:   # the flag may come with trailing arguments (blend_backward_splat_kernel: the AUX pointers)
            cand = [c for c in b if c not in a and c.startswith(k[:i] + "ELb0EEEv") and c.startswith(nk)]
            # ... or with a trailing parameter pack that is empty when the flag is false (geom_backward_kernel: the AA arrays)
            cand += [c for c in b if c not in a and c.startswith(k[:i] + "ELb0EJE" + k[i + 1:])]
            nk = cand[0] if len(cand) == 1 else nk
        if nk in b:
            renamed[k] = nk
            b[k] = b.pop(nk); new_name[k] = nk
# plain kernels that became templates on one flag (default false, trailing arguments if any): match "name(args" against "name<false>(args"
TEMPLATED = ("preprocess_kernel", "camera_partials_kernel")
def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: d.replace("void ", "", 1) if d.startswith("void ") else d for n, d in zip(names, out)}
gone_t = [k for k in a if k not in b and any(t in k for t in TEMPLATED)]
if gone_t:
    da, db = demangled(gone_t), demangled([c for c in b if c not in a])
    for k in gone_t:
        head = da[k][:-1]     # without the closing parenthesis
        cand = [c for c, d in db.items() if any(d.replace(t + "<false>", t) .startswith(head) and t + "<false>" in d for t in TEMPLATED)]
        if len(cand) == 1:
            renamed[k] = cand[0]
            b[k] = b.pop(cand[0]); new_name[k] = cand[0]
if pairs:
    b_new = {v: b[k] for k, v in new_name.items() if k in b}   # the new build by its own symbols
    da, db = demangled([k for k in a if k not in b]), demangled(list(b_new))
    paired = set()
    for old_text, new_text in pairs:
        olds, news = [k for k, d in da.items() if old_text in d], [k for k, d in db.items() if new_text in d]
        if len(olds) != 1 or len(news) != 1:
            sys.exit("--pair %s=%s: %d old and %d new kernels match" % (old_text, new_text, len(olds), len(news)))
        renamed[olds[0]] = news[0]
        b[olds[0]] = b_new[news[0]]; new_name[olds[0]] = news[0]; paired.add(news[0])
    for k in paired:
        if k in b and k not in a: del b[k]
print("renamed (old -> old + trailing flag = false):", len(renamed))
same = [k for k in a if k in b and a[k] == b[k]]
diff = [k for k in a if k in b and a[k] != b[k]]
gone = [k for k in a if k not in b]
new = [k for k in b if k not in a]
print(json.dumps({"symbols_before": len(a), "identical": len(same), "differ": diff, "removed": gone, "added": new}, indent=1))
for k in diff:
    ra, rb = dict(META[(sys.argv[1], k)], insts=len(a[k].splitlines())), dict(META[(sys.argv[2], new_name[k])], insts=len(b[k].splitlines()))
    print("differs: %s\n  old %s\n  new %s%s" % (demangled([k])[k], json.dumps(ra), json.dumps(rb), "   RISES: " + ", ".join(q for q in ra if rb[q] > ra[q]) if any(rb[q] > ra[q] for q in ra) else ""))
if len(sys.argv) > 3:
    import difflib
    for k in [k for t in sys.argv[3:] for k in diff if t in k]:   # SYMBOL: any part of a differing kernel's mangled name
        print("\n".join(list(difflib.unified_diff(a[k].splitlines(), b[k].splitlines(), lineterm="", n=1))[:int(os.environ.get("DIFF_LINES", "60"))]))
