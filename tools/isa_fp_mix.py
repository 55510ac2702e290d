#!/usr/bin/env python3
"""Floating-point instruction mix of kernels in an ISA listing (hipcc -S --cuda-device-only).

    tools/isa_fp_mix.py listing.s ba_backsub_kernel [more name fragments]

Prints, per kernel whose mangled name contains a fragment, the number of v_fma / v_mul / v_add (and v_sub) /
v_cvt / v_rcp / v_div operations by type suffix (v_fmac / v_fmamk / v_fmaak count as v_fma, a v_pk_* as two).  Two builds round alike only if these lines are equal:
a changed count means a multiply-add was contracted (or split) differently.
"""
import collections
import re
import sys

ALIAS = {"v_fmac": "v_fma", "v_fmamk": "v_fma", "v_fmaak": "v_fma", "v_mad": "v_fma", "v_mac": "v_fma"}
OPS = ("v_fma", "v_fmac", "v_fmamk", "v_fmaak", "v_mad", "v_mac", "v_mul", "v_add", "v_sub", "v_cvt", "v_rcp", "v_rsq", "v_sqrt", "v_div",
       "v_pk_fma", "v_pk_mul", "v_pk_add", "v_trig", "v_sin", "v_cos", "v_exp", "v_log", "v_ldexp", "v_frexp", "v_fract",
       "v_rndne", "v_floor", "v_trunc")
FP = re.compile(r"_(f16|f32|f64|bf16)(?=_|$)")


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name and line.startswith(".Lfunc_end"):  # (a kernel may hold several s_endpgm: early returns)
            yield name, body
            name = None
        elif name:
            body.append(line)


def mix(body):
    c = collections.Counter()
    for line in body:
        tok = line.split()
        if not tok or not tok[0].startswith("v_"):
            continue
        op = tok[0]
        if not FP.search(op):
            continue
        # longest matching prefix names the class
        cls = max((o for o in OPS if op.startswith(o + "_")), key=len, default=None)
        if cls:
            # one class for the encodings of a fused multiply-add; a packed instruction is two operations
            pk = 2 if cls.startswith("v_pk_") else 1
            cls = ALIAS.get(cls.replace("v_pk_", "v_"), cls.replace("v_pk_", "v_"))
            c[cls + "".join("_" + t for t in FP.findall(op))] += pk
    return c


def main():
    path, frags = sys.argv[1], sys.argv[2:]
    for name, body in kernels(path):
        if frags and not any(f in name for f in frags):
            continue
        c = mix(body)
        print(name)
        print("  " + "  ".join(f"{k}={c[k]}" for k in sorted(c)))


if __name__ == "__main__":
    main()
