#!/usr/bin/env python3
"""The PEELED form of k_shade's terminal iteration, as an experiment (measured and not kept: profiles/terminal_iteration_ab.txt).

The committed kernel decides with uniform run-time branches whether its last iteration runs in the terminal form (RenderParams::terminal).  This script writes a
copy of mitsuba3dopplertof_amd/csrc in which the body of the bounce loop is compiled TWICE instead -- once with `terminal` a compile-time 1 (the last iteration
of a terminal launch), once with 0 -- by moving the body into dtof_shade_bounce.inc and including it in both arms of one uniform branch.  (Wrapping the body in
a generic lambda with the form as a template argument, which a -D switch could select, was tried first: the captures by reference cost the traversal-stack
pointer its LDS address space, and the stack columns went to scratch.)

    python tools/experiments/terminal_peel.py OUT_DIR
    make -C OUT_DIR/mitsuba3dopplertof_amd/csrc -j8 ../libdtof.so        # then: tools/gpu_session.sh ab ... peel=<that library>
"""
import os
import shutil
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    out = sys.argv[1]
    src, dst = os.path.join(HERE, "mitsuba3dopplertof_amd", "csrc"), os.path.join(out, "mitsuba3dopplertof_amd", "csrc")
    os.makedirs(dst, exist_ok=True)
    for f in os.listdir(src):
        if f.endswith((".hip", ".h", ".cpp")) or f == "Makefile":
            shutil.copy(os.path.join(src, f), dst)
    shutil.copytree(os.path.join(HERE, "include"), os.path.join(out, "include"), dirs_exist_ok=True)
    lines = open(os.path.join(dst, "dtof_shade.h")).read().split("\n")
    a = next(i for i, l in enumerate(lines) if l.startswith("    for (uint32_t it = 0; ; ++it) {"))
    b = next(i for i, l in enumerate(lines) if l.strip() == "if (last) break;")
    swaps = {"    const bool last = it + 1 >= n_inline;": "    const bool last = DTOF_TERM ? true : last_rt;",
             "    const uint32_t trace_next = last ? trace_next_last : 1u;": "    const uint32_t trace_next = DTOF_TERM ? 0u : (last ? trace_next_last : 1u);",
             "    const bool terminal = last && rp.terminal != 0;": "    const bool terminal = DTOF_TERM != 0;"}
    body, done = [], 0
    for l in lines[a + 1:b]:
        for old, new in swaps.items():
            if l.startswith(old):
                l, done = new, done + 1
        body.append(l)
    assert done == len(swaps), "the bounce loop of dtof_shade.h no longer has the shape this script was written for"
    open(os.path.join(dst, "dtof_shade_bounce.inc"), "w").write("\n".join(body) + "\n")
    both = ["    const bool last_rt = it + 1 >= n_inline;", "    if (last_rt && rp.terminal != 0) {", "#define DTOF_TERM 1", '#include "dtof_shade_bounce.inc"', "#undef DTOF_TERM",
            "    } else {", "#define DTOF_TERM 0", '#include "dtof_shade_bounce.inc"', "#undef DTOF_TERM", "    }", "    const bool last = last_rt;"]
    open(os.path.join(dst, "dtof_shade.h"), "w").write("\n".join(lines[:a + 1] + both + lines[b:]))
    mk = open(os.path.join(dst, "Makefile")).read().replace("KERNEL_HDRS := ", "KERNEL_HDRS := dtof_shade_bounce.inc ", 1)
    open(os.path.join(dst, "Makefile"), "w").write(mk)
    print("peeled sources in", dst)


if __name__ == "__main__":
    main()
