#!/usr/bin/env python3
"""Developer tool (no GPU needed): which VALU instructions of a kernel take an SGPR as a source.
   python scripts/valu_operand_audit.py loss_fused.hip [project.hip optim.hip ...] [--kernels REGEX] [--list]
Compiles each given file of brush_amd/csrc/ to gfx950 assembly with the Makefile's HIPFLAGS and prints, per kernel: VGPRs, LDS
bytes, scratch, waves per SIMD (the compiler's own occupancy figure), VALU instructions, how many of them have an SGPR source, and
the float multiply / FMA family on its own.  By the cost model of DESIGN.md §4 (scripts/micro/valu_rates.hip) an SGPR source halves
a VALU op's issue rate.  Static counts of the whole kernel body: a loop counts once, whatever its trip count.

What counts as an SGPR source: s<N> / s[N:M] / ttmp among the operands BEHIND the destination(s).  The lane mask of v_cndmask and
the carry-in of add-with-carry are not counted (they cannot live anywhere else), nor are vcc / exec / inline constants / literals.
--list prints the counted instructions.  The tool only classifies operand kinds."""
import argparse, collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "brush_amd", "csrc")
SREG = re.compile(r"^-?\|?(s\d+|s\[\d+:\d+\]|ttmp\d+|ttmp\[\d+:\d+\])\|?$")
FMUL = re.compile(r"^v_(pk_)?(mul|fma|fmac|mad|mac|fmamk|fmaak)(_legacy)?_f(16|32|64)")
TWO_DST = re.compile(r"^v_(add_co|sub_co|subrev_co|addc_co|subb_co|subbrev_co|mad_u64_u32|mad_i64_i32|div_scale)")
MASK_LAST = re.compile(r"^v_(cndmask|addc_co|subb_co|subbrev_co)")


def makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1)
    return hipcc, flags


def demangle(names):
    filt = os.path.join(os.path.dirname(os.path.realpath(makefile_flags()[0])), "..", "llvm", "bin", "llvm-cxxfilt")
    for tool in (filt, "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def sources(op, operands):
    ops = [o.strip() for o in re.split(r",(?![^\[]*\])", operands) if o.strip()]
    ops = [o for o in ops if not re.match(r"^(op_sel|op_sel_hi|neg_lo|neg_hi|clamp|mul:|div:|row_|quad_perm|bank_mask|row_mask|bound_ctrl|dst_sel|src\d_sel|dst_unused|fi:)", o)]
    ops = [o.split(" ")[0] for o in ops]
    base = re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", op)
    src = ops[2 if TWO_DST.match(base) else 1:]
    if MASK_LAST.match(base) and src and (SREG.match(src[-1]) or src[-1] in ("vcc", "vcc_lo")):
        src = src[:-1]
    return src


def audit(asm):
    """[(mangled name, info dict)] for every kernel (a function followed by an .amdhsa_kernel block) of the assembly text."""
    lines = asm.split("\n")
    kernels = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", l)] if m]
    out = []
    for k in kernels:
        start = next(i for i, l in enumerate(lines) if l.startswith(k + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        info = collections.OrderedDict(vgprs=None, agprs=None, lds=None, scratch=None, waves=None)
        for l in lines[end:end + 80]:
            for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
                             ("waves", r"; Occupancy: (\d+)")):
                m = re.match(pat, l)
                if m and info[key] is None:
                    info[key] = int(m.group(1))
        valu = sg = fm = fm_sg = 0
        hits = []
        for l in lines[start + 1:end]:
            t = l.strip()
            if not t.startswith("v_"):
                continue
            t = t.split(";")[0].strip()
            op, _, rest = t.partition(" ")
            if op.startswith("v_nop"):
                continue
            valu += 1
            has = any(SREG.match(s) for s in sources(op, rest))
            isf = bool(FMUL.match(op))
            sg += has
            fm += isf
            fm_sg += has and isf
            if has:
                hits.append(t)
        info.update(valu=valu, valu_sgpr=sg, fmul=fm, fmul_sgpr=fm_sg, hits=hits)
        out.append((k, info))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="+", help="files of brush_amd/csrc/ (or paths)")
    ap.add_argument("--kernels", default="", help="only kernels whose demangled name matches this regex")
    ap.add_argument("--list", action="store_true", help="also print every instruction counted as having an SGPR source")
    args = ap.parse_args()
    hipcc, flags = makefile_flags()
    print("# %s %s -S --cuda-device-only" % (os.path.basename(hipcc), " ".join(flags)))
    print("# %-72s %5s %7s %7s %5s %6s %9s %8s %11s" % ("kernel", "VGPRs", "LDS B", "scratch", "waves", "VALU", "SGPR src", "mul/FMA", "..SGPR src"))
    for f in args.files:
        src = f if os.path.exists(f) else os.path.join(CSRC, f)
        with tempfile.TemporaryDirectory() as td:
            asm = os.path.join(td, "a.s")
            subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", "-I" + CSRC, src, "-o", asm], stderr=subprocess.DEVNULL)
            res = audit(open(asm).read())
        names = demangle([k for k, _ in res])
        print("## " + os.path.basename(src))
        for k, i in res:
            name = re.sub(r"\(anonymous namespace\)::", "", names[k]).replace("bh::", "")
            name = re.sub(r"\(.*\)$", "", name).replace("void ", "")
            if args.kernels and not re.search(args.kernels, name):
                continue
            print("%-74s %5d %7d %7d %5d %6d %9d %8d %11d" % (name[:74], i["vgprs"] + (i["agprs"] or 0), i["lds"], i["scratch"], i["waves"], i["valu"], i["valu_sgpr"],
                                                             i["fmul"], i["fmul_sgpr"]))
            if args.list:
                for h in i["hits"]:
                    print("      " + h)
    return 0


if __name__ == "__main__":
    sys.exit(main())
