"""Which kernels of one translation unit compile to the same device code in two trees?

    hipcc <the flags of csrc/build.py> --cuda-device-only -S csrc/headloss.hip -o before.s   (old tree)
    hipcc <the flags of csrc/build.py> --cuda-device-only -S csrc/headloss.hip -o after.s    (new tree)
    python tools/compare_kernel_asm.py before.s after.s [--drop ', true>(']

Splits both gfx950 assembly files into kernels, demangles the names, strips comments, local labels
and the kernel's own symbol, and compares the instruction streams kernel by kernel.  --drop removes
a substring from the demangled names of the NEW file before matching: a template parameter added
with a value that selects the old behaviour (k_box_ml<float, false, true> matches the old
k_box_ml<float, false>).  Kernels of the new file without a partner are listed as new instances.
Exit status 1 when a kernel of the old file is missing or differs.
"""
import re
import subprocess
import sys


def kernels(path):
    txt = open(path).read()
    return {m.group(1): m.group(2) for m in
            re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel', txt, re.S | re.M)}


def demangle(names):
    """mangled -> demangled name; the parameter list is reduced to '()': kernel name and template
    arguments identify an instance, and a parameter type that came to depend on a new template
    parameter (k_focal_ml's argument block) must not hide the old instance's partner"""
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True,
                         text=True).stdout.split('\n')
    return dict(zip(names, (re.sub(r'>\(.*\)$', '>()', o) for o in out)))


def stream(body, name):
    body = re.sub(r';.*', '', body.replace(name, 'KERNEL'))
    body = re.sub(r'\.L\w+', '.L', body)
    return [ln.strip() for ln in body.split('\n') if ln.strip()]


if __name__ == '__main__':
    args = sys.argv[1:]
    drop = None
    if '--drop' in args:
        k = args.index('--drop')
        drop = args[k + 1]
        del args[k:k + 2]
    old, new = kernels(args[0]), kernels(args[1])
    d_old, d_new = demangle(list(old)), demangle(list(new))
    # a new kernel whose own name exists in the old file is its partner; --drop applies to the rest
    old_names = set(d_old.values())
    by_name = {}
    for n in new:
        name = d_new[n]
        if name not in old_names and drop and drop in name:
            name = name.replace(drop, '>(')
        by_name[name] = n
    bad = 0
    for n in old:
        m = by_name.pop(d_old[n], None)
        same = m is not None and stream(old[n], n) == stream(new[m], m)
        print('%-9s %s' % ('identical' if same else ('MISSING' if m is None else 'DIFFERENT'), d_old[n]))
        bad += not same
    for name in sorted(by_name):
        print('new       %s' % d_new[by_name[name]])
    sys.exit(1 if bad else 0)
