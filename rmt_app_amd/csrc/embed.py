#!/usr/bin/env python3
"""Concatenate the device template's parts (kernels/ORDER) and wrap the text into a C++ raw string
literal (n2_kernels_embed.h) for rmt_n2.cpp.  `embed.py --cat` prints the template itself;
`embed.py --file SOURCE OUT` wraps one file the same way (the monitor's translation unit)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def parts():
    out = []
    for line in open(os.path.join(HERE, "kernels", "ORDER")):
        name = line.split("#", 1)[0].strip()
        if name:
            out.append(os.path.join(HERE, "kernels", name))
    return out


def template():
    return "".join(open(p).read() for p in parts())


if __name__ == "__main__":
    if sys.argv[1] == "--file":
        text, out = open(os.path.join(HERE, sys.argv[2])).read(), sys.argv[3]
    else:
        text, out = template(), sys.argv[1]
    if out == "--cat":
        sys.stdout.write(text)
    else:
        assert ')RMTSRC"' not in text
        with open(out, "w") as f:
            f.write('R"RMTSRC(' + text + ')RMTSRC"\n')
