"""Per-kernel comparison of two gfx950 device-assembly files written by tools/device_asm.sh: every function body (label to
.Lfunc_endN) and every .amdhsa_kernel descriptor (registers, LDS, scratch), with the function-numbered labels that adding or
removing a kernel renumbers (BB<n>_, .Ltmp<n>, .Lfunc_end<n>) normalised.  Exit status 1 when a kernel present in both differs
or the second file has one the first has not.
    python tools/asm_compare.py base.s new.s"""
import re
import sys


def kernels(path):
    txt, out = open(path).read(), {}
    for m in re.finditer(r'^([_a-zA-Z]\S*):\s*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:', txt, re.S | re.M):
        body = re.sub(r'BB\d+_', 'BB_', m.group(2))
        body = re.sub(r'\.Ltmp\d+', '.Ltmp', body)
        out[m.group(1)] = re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', body)
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', txt, re.S | re.M):
        out[m.group(1) + '#kd'] = m.group(2)
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    diff = sorted(k for k in a if k in b and a[k] != b[k])
    print('gone:', sorted(k for k in set(a) - set(b) if not k.endswith('#kd')), 'new:', sorted(set(b) - set(a)), 'differing:', len(diff), diff)
    sys.exit(1 if diff or set(b) - set(a) else 0)
