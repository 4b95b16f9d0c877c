#!/usr/bin/env python3
"""Generate tests/golden/bior_taps.json: the stored low-pass arrays of the reference's biorthogonal families.

Reads the text of the reference's ``BiorthogonalSpline.java`` (vectorwave-core/src/main/java/com/morphiqlabs/
wavelet/api/), evaluates its ``private static final double`` constants the way Java does (IEEE double division
and Math.sqrt) and every ``new double[]{...}`` of the BIORx_y declarations, and writes

    {"bior1.1": {"dec": ["0x1.6a09e667f3bcdp-1", ...], "rec": [...]}, ..., "rbio1.1": {...}, ...}

name -> the two stored arrays (lowPassDecomposition, lowPassReconstruction) as hex-float strings; the rbio
entries are their bior originals with the two arrays swapped (ReverseBiorthogonalSpline.java:107-128).  Data only.
tests/test_bior_catalogue_cpu.py compares vectorwave_amd.wavelets with this file bit for bit.

    python tests/golden/make_bior_fixture.py <path to the reference checkout>
"""
import json
import math
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
JAVA = "vectorwave-core/src/main/java/com/morphiqlabs/wavelet/api/BiorthogonalSpline.java"


def _strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _value(expr: str, consts: dict) -> float:
    """A Java constant expression of doubles: literals, names, unary minus, /, Math.sqrt."""
    expr = expr.strip().replace("Math.sqrt", "math.sqrt")
    if not re.fullmatch(r"[\w\s.+\-*/()]+", expr):
        raise ValueError(f"unexpected expression {expr!r}")
    return float(eval(expr, {"__builtins__": {}, "math": math}, dict(consts)))  # noqa: S307 (checked above)


def parse(text: str) -> dict:
    text = _strip_comments(text)
    consts = {}
    for name, expr in re.findall(r"private static final double (\w+)\s*=\s*([^;]+);", text):
        consts[name] = _value(expr, consts)
    out = {}
    decl = re.compile(r'new BiorthogonalSpline\(\s*"([^"]+)"\s*,\s*\d+\s*,\s*\d+\s*,\s*new double\[\]\{([^}]*)\}\s*,'
                      r"\s*new double\[\]\{([^}]*)\}", re.S)
    for name, dec, rec in decl.findall(text):
        out[name] = {k: [_value(e, consts) for e in arr.split(",")] for k, arr in (("dec", dec), ("rec", rec))}
    return out


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with open(os.path.join(sys.argv[1], JAVA)) as f:
        bior = parse(f.read())
    if len(bior) != 15:
        sys.exit(f"expected 15 BIOR declarations, found {len(bior)}")
    table = {}
    for name, t in bior.items():
        table[name] = {"dec": [v.hex() for v in t["dec"]], "rec": [v.hex() for v in t["rec"]]}
    for name, t in bior.items():
        table["rbio" + name[4:]] = {"dec": [v.hex() for v in t["rec"]], "rec": [v.hex() for v in t["dec"]]}
    path = os.path.join(HERE, "bior_taps.json")
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(table)} wavelets")


if __name__ == "__main__":
    main()
