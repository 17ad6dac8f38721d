"""Static instruction / scratch counts of the lean twin of the log-derivative camera kernel (csrc/psdr_logd_lean.h, psdr_logd_lean.hip), pinned.

The twin exists to keep a path's idle state out of scratch memory: k_camera_logd<1, 8, true> carries 71 scratch instructions (tests/golden/isa_counts.json), and the
twin must stay strictly below that -- whatever else moves.  Like tests/test_isa_guard.py this disassembles the BUILT library and compares with a table
(tests/golden/logd_lean_isa.json): +-1 % instructions, no new scratch instruction.  A deliberate change regenerates the table:
python tests/test_logd_lean_isa.py --write  (and says so in the commit).
CPU test: reads psdr-cuda_amd/lib/obj/logd_lean.o (what build() leaves here) or, without the object, the code objects inside libpsdr_hip.so.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TABLE = os.path.join(ROOT, "tests", "golden", "logd_lean_isa.json")
PARENT_TABLE = os.path.join(ROOT, "tests", "golden", "isa_counts.json")
KERNELS = {
    "k_camera_logd_lean<1, 8, false>": "C2 renderD forward K = 1, lean twin seeding its streams itself",
    "k_camera_logd_lean<1, 8, true>": "C2 renderD forward K = 1, lean twin loading its seeds (the headline's renderD kernel)",
}


def disassemble():
    import check_spill_exec as cse
    objdump = cse.find_objdump()
    lib = os.path.join(ROOT, "psdr-cuda_amd", "lib", "libpsdr_hip.so")
    o = os.path.join(ROOT, "psdr-cuda_amd", "lib", "obj", "logd_lean.o")
    blobs = []
    if os.path.exists(o) and os.path.getmtime(o) >= os.path.getmtime(lib) - 3600:
        blobs = cse.code_objects(o)
    if not blobs:
        blobs = cse.code_objects(lib)
    assert blobs, "no gfx950 code object found"
    out = {}
    for b in blobs:
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(b); f.flush()
            txt = subprocess.run([objdump, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for l in txt.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:", l)
            if m:
                cur = m.group(1) if "logd_lean" in m.group(1) else None
                if cur:
                    out.setdefault(cur, [0, 0, 0])
                continue
            if cur and re.match(r"^\s+[a-z]", l):
                ins = l.strip().split()[0]
                if ins.startswith("s_nop") or ins.startswith("s_code_end"):
                    continue
                out[cur][0] += 1
                out[cur][1] += 1 if ins.startswith("scratch_") else 0
                out[cur][2] += 1 if ins.startswith("ds_") else 0
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for mangled, dem in zip(out, names):
        short = dem.replace("(anonymous namespace)::", "").replace("psdr::", "").replace("void ", "").split("(")[0]
        if short in KERNELS and out[mangled][0] > 100:
            res[short] = {"instructions": out[mangled][0], "scratch": out[mangled][1], "lds": out[mangled][2]}
    return res


def test_the_lean_twin_keeps_its_counts_and_stays_below_the_scratch_instructions_of_the_kernel_it_replaces():
    now = disassemble()
    want = json.load(open(TABLE))
    parent = json.load(open(PARENT_TABLE))["k_camera_logd<1, 8, true>"]
    assert parent["scratch"] == 71
    missing = sorted(set(KERNELS) - set(now))
    assert not missing, "kernels not found in the library: %s" % missing
    bad = []
    for k in KERNELS:
        a, b = now[k], want[k]
        print("%s: %d instructions, %d scratch, %d LDS (table %d / %d / %d; k_camera_logd<1, 8, true> %d / %d)"
              % (k, a["instructions"], a["scratch"], a["lds"], b["instructions"], b["scratch"], b["lds"], parent["instructions"], parent["scratch"]))
        assert a["scratch"] < parent["scratch"], (k, a["scratch"], parent["scratch"])
        if abs(a["instructions"] - b["instructions"]) > 0.01 * b["instructions"] or a["scratch"] > b["scratch"]:
            bad.append("%s (%s): %d instructions / %d scratch, table %d / %d" % (k, KERNELS[k], a["instructions"], a["scratch"], b["instructions"], b["scratch"]))
    assert not bad, "kernels moved (a deliberate change regenerates the table: python tests/test_logd_lean_isa.py --write):\n  " + "\n  ".join(bad)


if __name__ == "__main__":
    if "--write" in sys.argv:
        json.dump(disassemble(), open(TABLE, "w"), indent=1, sort_keys=True)
    for k, v in sorted(disassemble().items()):
        print("%-36s %6d instructions %4d scratch %4d lds   %s" % (k, v["instructions"], v["scratch"], v["lds"], KERNELS[k]))
