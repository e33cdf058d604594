#!/usr/bin/env python3
"""Static resource usage of every kernel in the built objects of mitsuba3dopplertof_amd/csrc, read from the code objects' metadata notes, in the format of
profiles/variants_resource_usage.txt; with a second object directory (the parent commit's build, same compiler) every line that differs ends with the parent's values,
and the machine code of every kernel both builds have is compared instruction by instruction.
usage: kernel_resources.py OBJDIR [PARENT_OBJDIR] [--all]      (--all: every kernel, not only k_shade)
Occupancy (waves per SIMD) follows from the VGPR count as the compiler's resource remarks report it for gfx950: 512 registers per SIMD lane in blocks of 8, at most 8."""
import os, re, shutil, subprocess, sys, tempfile
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
UNITS = ["dtof_kernels", "dtof_shade_plain", "dtof_shade_mesh", "dtof_shade_spec1", "dtof_shade_spec2", "dtof_shade_res0", "dtof_shade_res1", "dtof_shade_res2",
         "dtof_film64", "dtof_moments", "dtof_aov", "dtof_develop", "dtof_adaptive"]
FIELDS = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("vspill", ".vgpr_spill_count"), ("sspill", ".sgpr_spill_count"),
          ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size")]


# (RESW, mask) of the specialised instantiations with the default -D values: the C2 / C3 kernels of dtof_shade_plain.hip and the resident Domino kernel of dtof_shade_res0.hip
FACT_MASKS = {("0", 0x52fffff): " = kHeadlinePairFacts", ("0", 0x12fffff): " = kHeadlineShapeFacts", ("0", 0x3ffff): " = kHeadlineC2Facts", ("0", 0x1fff): " = kHeadlineFusedFacts", ("0", 0xfff): " = kHeadlineFacts", ("16", 0x37f): " = kResidentFacts"}


def run(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def kernels(objdir, tmp, tag):
    """{demangled name: (resources, [instructions])} over the kernel objects of one build"""
    out = {}
    for u in UNITS:
        fat, co = os.path.join(tmp, "%s_%s.fatbin" % (tag, u)), os.path.join(tmp, "%s_%s.co" % (tag, u))
        run(LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", os.path.join(objdir, u + ".o"), fat)
        run(LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co)
        text = {}
        cur = None
        for ln in run(LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).split("\n"):
            m = re.match(r"^[0-9a-f]* ?<(\w+)>:", ln)
            if m:
                cur = text.setdefault(m.group(1), [])
            elif cur is not None and ln.strip():
                cur.append(ln.split("//")[0].strip())
        for rec in run(LLVM + "/llvm-readelf", "--notes", co).split("  - .agpr_count:")[1:]:
            rec = ".agpr_count:" + rec
            get = lambda k: re.search(r"^\s*%s:\s*(\S+)" % re.escape(k), rec, re.M)
            sym = re.sub(r"\.kd$", "", get(".symbol").group(1).strip("'"))
            res = {n: int(get(k).group(1)) if get(k) else 0 for n, k in FIELDS}
            res["occ"] = min(8, 512 // max(8, (res["vgpr"] + res["agpr"] + 7) // 8 * 8))
            name = run(shutil.which("c++filt") or LLVM + "/llvm-cxxfilt", sym).strip().replace("(anonymous namespace)::", "").replace("void dtof::", "").split("(")[0]
            name = re.sub(r", 0u>$", ">", name)   # FACTS = 0 (k_shade's last template argument): the name the kernel had without it
            m = re.search(r", (\d+)u>$", name)      # ... and a kernel compiled with plan facts (dtof_kernels.h: kFact*): its mask in hex, with the name of the mask
            if m and name.startswith("k_shade<"):
                name = name[:m.start()] + ", FACTS 0x%x%s>" % (int(m.group(1)), FACT_MASKS.get((name.split(", ")[6], int(m.group(1))), ""))
            out[name] = (res, text.get(sym, []))
    return out


def line(res):
    return " ".join("%s %4d" % (k, res[k]) for k in ("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "occ", "lds"))


def main():
    args = [a for a in sys.argv[1:] if a != "--all"]
    every = "--all" in sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        new = kernels(args[0], tmp, "new")
        old = kernels(args[1], tmp, "parent") if len(args) > 1 else None
    names = sorted(n for n in new if every or n.startswith("k_shade<"))
    n_res = n_text = 0
    for n in names:
        res, text = new[n]
        note = ""
        if old is not None:
            if n not in old:
                note = "   <-- new"
            else:
                pres, ptext = old[n]
                diff = ["%s %d" % (k, pres[k]) for k in pres if pres[k] != res[k]]
                if diff:
                    note, n_res = "   <-- parent: " + ", ".join(diff), n_res + 1
                if ptext != text:
                    note, n_text = note + "   (machine code differs: %d -> %d instructions)" % (len(ptext), len(text)), n_text + 1
        print("%-78s %s%s" % (n, line(res), note))
    if old is not None:
        print("\n%d kernels listed; %d not in the parent build; %d differ from the parent in a resource figure, %d in their machine code; %d of the parent's are gone"
              % (len(names), sum(n not in old for n in names), n_res, n_text, sum((every or n.startswith("k_shade<")) and n not in new for n in old)))


if __name__ == "__main__":
    main()
