"""Per-kernel VGPR / spill / scratch counts of a HIP source for gfx950 (device-only asm, no GPU
needed), and with --fp64 each kernel's fp64 VALU instruction multiset (two instantiations compute
the same arithmetic only if the compiler contracted them alike: compare their multisets).
A -DNAME argument goes to the compiler (assemble.hip's -DASM_REGULAR_CHECK: the regular walk
alone in its kernels, next to the general walk unrolled for six neighbours).
usage: python tools/isa_regs.py dune-pnp_amd/csrc/assemble.hip [name-filter] [--fp64] [-DNAME]"""
import collections
import re
import subprocess
import sys

defs = [a for a in sys.argv[1:] if a.startswith("-D")]
args = [a for a in sys.argv[1:] if a != "--fp64" and a not in defs]
fp64 = "--fp64" in sys.argv[1:]
src = args[0]
filt = args[1] if len(args) > 1 else ""
out = "/tmp/isa_regs.s"
subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                       "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-o", out, src] + defs,
                      stderr=subprocess.DEVNULL)
txt = open(out).read()


def bodies(text):
    """mangled kernel name -> its instruction lines"""
    res, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = res.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            cur.append(line.strip())
    return res


code = bodies(txt) if fp64 else {}
meta = txt[txt.index("amdhsa.kernels"):]
for blk in re.split(r"\n  - ", meta)[1:]:
    g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
    name = subprocess.run(["c++filt"], input=g("name"), capture_output=True, text=True).stdout.strip()
    if filt in name:
        print(f"vgpr={g('vgpr_count'):>4} spill={g('vgpr_spill_count'):>3} "
              f"scratch={g('private_segment_fixed_size'):>4} "
              f"lds={g('group_segment_fixed_size'):>6}  {name[:110]}")
        if fp64:
            ops = collections.Counter(re.match(r"(v_\w+_f64)", l).group(1)
                                      for l in code.get(g("name"), [])
                                      if re.match(r"v_\w+_f64", l))
            print("      fp64: " + ", ".join(f"{v} {k}" for k, v in sorted(ops.items())))
