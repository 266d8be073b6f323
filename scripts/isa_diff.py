#!/usr/bin/env python3
"""Compare the gfx950 device assembly of csrc/kernels/*.hip, kernel by kernel, between a git
revision and the working tree, for the default and the -DSL_DETERMINISTIC=1 build.  Text only.

  scripts/isa_diff.py [REV] [old=new ...] [--loose | --mix]

Prints SAME / DIFF / GONE / NEW per kernel; exits 1 on any DIFF or NEW.  `old=new` maps a
renamed (mangled) kernel, such as one that became a template instantiation; the section a kernel
is placed in (a template's own comdat section) is not compared.  --loose is the check for a kernel
whose parameter list changed: the scalar kernarg loads, waits and scalar register numbers are
dropped and, of the descriptor, only VGPR count, accum offset and private segment size must be
equal and the LDS size no larger.
--mix is the check for a kernel whose source was rearranged without changing what it does: those
descriptor fields again, and the number of instructions in each of the classes MUST (matrix, LDS,
buffer and global loads / stores / atomics, barriers) must be equal; such a kernel prints MIX with
its VALU, SALU and s_waitcnt counts as old -> new, which do not fail the check.
"""
import concurrent.futures as cf, glob, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result",
         "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", "-o", "-"]
NORM = [(r"__hip_cuid_\w+", "__hip_cuid"), (r"(\.LBB|\.Lfunc_end|BB)\d+", r"\1"), (r"\s*;.*", ""),
        (r"(?m)^\s*\.(text|section)\b.*", "")]  # where the code is placed (a template's comdat section) is not code
KEEP = ("next_free_vgpr", "accum_offset", "private_segment_fixed_size")
MUST = ("v_mfma", "ds_", "buffer_load", "buffer_store", "buffer_atomic", "global_load", "global_store", "global_atomic",
        "buffer_", "global_", "s_barrier")  # first match: the bare buffer_ / global_ count the rest (cache control)
SHOWN = ("valu", "salu", "s_waitcnt")


def mix(body, desc):
    """descriptor fields and instruction counts by class of one kernel's text"""
    out = {k: re.search(k + r"\s+(\d+)", desc).group(1) for k in KEEP}
    out.update(dict.fromkeys(MUST + SHOWN, 0))
    for l in body.splitlines():
        op = re.match(r"\s+([vs]_\w+|ds_\w+|buffer_\w+|global_\w+)", l)
        if not op:
            continue
        op = op.group(1)
        cls = next((c for c in MUST + ("s_waitcnt",) if op.startswith(c)), "valu" if op[0] == "v" else "salu" if op[0] == "s" else None)
        out[cls] += 1
    return out


def kernels(src, det, loose):
    """{name: (normalised text, LDS bytes, mix)} of one source file: each function body plus its descriptor"""
    cmd = ["hipcc", *FLAGS, "-I" + os.path.dirname(src), src] + (["-DSL_DETERMINISTIC=1"] if det else [])
    asm = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n.*?^\.Lfunc_end\d+:", asm, re.S | re.M):
        desc = re.search(r"^\s*\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % m.group(1), asm, re.S | re.M)
        desc = desc.group(0) if desc else ""
        body = m.group(0).replace(desc, "")  # the descriptor sits inside the function's span
        lds = re.search(r"group_segment_fixed_size (\d+)", desc)
        counts = mix(body, desc)
        if loose:
            body = "\n".join(l for l in body.splitlines() if not re.match(r"\s*s_(load|waitcnt)", l))
            body = re.sub(r"\bs(\d+|\[\d+:\d+\])", "s", body)
            desc = "\n".join(l.strip() for l in desc.splitlines() if any(k in l for k in KEEP))
        text = body + "\n" + desc
        for pat, rep in NORM:
            text = re.sub(pat, rep, text)
        out[m.group(1)] = ("\n".join(l.rstrip() for l in text.splitlines() if l.strip()), int(lds.group(1)) if lds else 0, counts)
    return out


def main(argv):
    loose, mixed = "--loose" in argv, "--mix" in argv
    argv = [a for a in argv if a not in ("--loose", "--mix")]
    rename = dict(a.split("=") for a in argv if "=" in a)
    rev = ([a for a in argv if "=" not in a] or ["HEAD"])[0]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(16) as pool:
        subprocess.run("git archive %s csrc/kernels | tar -x -C %s" % (rev, tmp), shell=True, check=True, cwd=ROOT)
        for det in (False, True):
            side = []
            for root in (tmp, ROOT):
                srcs = sorted(glob.glob(os.path.join(root, "csrc", "kernels", "*.hip")))
                side.append((srcs, [pool.submit(kernels, s, det, loose) for s in srcs]))
            old, new = ({k: (os.path.basename(s), v) for s, f in zip(*sd) for k, v in f.result().items()} for sd in side)
            old = {rename.get(k, k): (f, v) for k, (f, v) in old.items()}
            for k in sorted(set(old) | set(new)):
                f, a = old.get(k, (None, None))
                f, b = new.get(k, (f, None))
                was = next((o for o, n in rename.items() if n == k), k)  # the name the old text carries
                same = a and b and a[0] == b[0].replace(k, was) and b[1] <= a[1]
                verdict = "GONE" if b is None else "NEW" if a is None else "SAME" if same else "DIFF"
                note = ""
                if mixed and verdict == "DIFF":
                    if b[1] <= a[1] and all(a[2][c] == b[2][c] for c in KEEP + MUST):
                        verdict = "MIX"
                    note = "\n       lds %d -> %d  " % (a[1], b[1]) + "  ".join(
                        "%s %s" % (c, a[2][c]) if a[2][c] == b[2][c] else "%s %s -> %s" % (c, a[2][c], b[2][c])
                        for c in KEEP + MUST + SHOWN if a[2][c] or b[2][c])
                bad += verdict in ("DIFF", "NEW")
                print("%-4s %-7s %-18s %s%s" % (verdict, "det" if det else "default", f, k, note))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
