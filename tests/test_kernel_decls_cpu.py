"""CPU: no .hip file declares a kernel by hand.  The kernels have C linkage, so a declaration that disagrees with the definition links and launches with the wrong
argument bytes; csrc/zkc_kernels.h declares every cross-file kernel once and is included by the launching files and by the defining file, where a disagreement
fails to compile."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'zk-franchise-proof-circuit_amd', 'csrc')
# extern "C" __global__ <anything but a body or another statement> ( parameters ) ;
DECL = re.compile(r'extern\s+"C"\s+__global__[^;{]*\([^;{]*\)\s*;')


def test_kernel_declarations_live_in_the_header_only():
    srcs = sorted(glob.glob(os.path.join(CSRC, '*.hip')))
    assert len(srcs) >= 10
    found = {os.path.basename(p): [m.group(0).split('(')[0].split()[-1] for m in DECL.finditer(open(p).read())] for p in srcs}
    assert {f: names for f, names in found.items() if names} == {}
    header = open(os.path.join(CSRC, 'zkc_kernels.h')).read()
    declared = [m.group(0).split('(')[0].split()[-1] for m in DECL.finditer(header)]
    assert len(declared) == len(set(declared)) >= 19
    # the header is included where its kernels are defined (that is what turns a mismatch into a compile error) and where they are launched
    for p in srcs:
        text = open(p).read()
        if any(re.search(r'\b%s\b' % k, text) for k in declared):
            assert '#include "zkc_kernels.h"' in text, os.path.basename(p)
