#!/usr/bin/env python3
"""Compare the gfx950 machine code of every kernel symbol in two builds of libgsr_hip.so, symbol by symbol:
    python tools/kernel_disasm_diff.py OLD/libgsr_hip.so NEW/libgsr_hip.so [SYMBOL ...]   (SYMBOL: print that kernel's diff)
llvm-objdump disassembles each offload bundle; branch targets, comments and inter-function padding are normalised away.
radix_scatter_kernel gained a trailing template flag CAP (capacity mode, default false), blend_backward_splat_kernel and
geom_backward_kernel one named AUX (include/gsr_aux_grads.h, default false; the blend kernel also two trailing pointer
arguments), and blend_backward_splat_kernel a second one named ABS behind it (include/gsr_densify_stats.h, default false, no new
arguments): an old instantiation is compared with its flag = false namesake.  Prints the counts and the symbols that differ, were removed or were added (JSON)."""
import glob, os, re, shutil, subprocess, sys, tempfile, json
OBJ = "/opt/rocm/llvm/bin/llvm-objdump"
def kernels(so):
    d = tempfile.mkdtemp()
    s = os.path.join(d, "lib.so"); shutil.copy(so, s)
    subprocess.run([OBJ, "--offloading", s], cwd=d, capture_output=True, check=True)
    out = {}
    for co in sorted(glob.glob(s + ".*gfx950")):
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
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
# kernels that gained a trailing template flag (default false): map each old instantiation to its flag=false name
FLAGGED = ("radix_scatter_kernelI", "blend_backward_splat_kernelI", "geom_backward_kernelI")
renamed = {}
for k in list(a):
    if k not in b and any(f in k for f in FLAGGED):
        i = k.index("EEEv")
        nk = k[:i] + "ELb0" + k[i:]
        if nk not in b:   # the flag may come with trailing arguments (blend_backward_splat_kernel: the AUX pointers)
            cand = [c for c in b if c not in a and c.startswith(k[:i] + "ELb0EEEv") and c.startswith(nk)]
            nk = cand[0] if len(cand) == 1 else nk
        if nk in b:
            renamed[k] = nk
            b[k] = b.pop(nk)
print("renamed (old -> old + trailing flag = false):", len(renamed))
same = [k for k in a if k in b and a[k] == b[k]]
diff = [k for k in a if k in b and a[k] != b[k]]
gone = [k for k in a if k not in b]
new = [k for k in b if k not in a]
print(json.dumps({"symbols_before": len(a), "identical": len(same), "differ": diff, "removed": gone, "added": new}, indent=1))
if len(sys.argv) > 3:
    import difflib
    for k in sys.argv[3:]:
        print("\n".join(list(difflib.unified_diff(a[k].splitlines(), b[k].splitlines(), lineterm="", n=1))[:60]))
