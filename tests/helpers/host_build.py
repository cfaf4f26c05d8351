"""Builds one of the stand-alone host programs of this directory (*_emu.cpp on rmt_host_unit.h) around the generated
source of a unit: the one compiler line the CPU tests of the march, profile, campaign, policy and sensitivity units share."""
import os
import subprocess


def build_helper(helper, src, tmp, tag, exe_name, sanitize=False):
    """Writes ``src`` to ``tmp``/unit_``tag``.inc, compiles ``helper`` around it into ``tmp``/``exe_name`` (contraction off;
    ``sanitize``: with AddressSanitizer and UBSan, every report fatal) and returns the program's path."""
    unit = os.path.join(tmp, "unit_%s.inc" % tag)
    with open(unit, "w") as f:
        f.write(src)
    exe = os.path.join(tmp, exe_name)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + san +
                   ["-DRMT_GENERATED_SOURCE=\"%s\"" % unit, helper, "-o", exe], check=True, capture_output=True)
    return exe
