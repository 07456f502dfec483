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


def test_host_helpers_are_defined_once_and_declared_in_headers():
    """The host-side helpers that several files used to carry private copies of exist once in csrc (zkc_host_util.h, zkc_internal.h), and no .hip file declares a function of
    another file by hand: those declarations live in zkc_internal.h, zkc_prover.h and the public header, where the defining file sees them too."""
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert len(files) >= 30
    text = {os.path.basename(p): open(p).read() for p in files}

    def definitions(pattern):
        return [(f, m.group(0)) for f, t in text.items() for m in re.finditer(pattern, t)]
    body = r'\s*\([^;{}]*\)\s*(?:const\s*)?\{'                                      # a parameter list followed by a body
    assert [f for f, _ in definitions(r'\b\w*root_of_unity' + body)] == ['zkc_host_util.h']
    assert [m.split('(')[0].split()[-1] for _, m in definitions(r'\b\w*root_of_unity' + body)] == ['fr_root_of_unity']
    assert [f for f, _ in definitions(r'\bg2_generator' + body)] == ['zkc_host_util.h']
    assert [f for f, _ in definitions(r'\bg1_generator' + body)] == ['zkc_host_util.h']
    assert [f for f, _ in definitions(r'\bstruct\s+DevBuf\b[^;{]*\{')] == ['zkc_internal.h']
    assert [f for f, _ in definitions(r'\berr_out' + body)] == ['zkc_host_util.h']
    # the millisecond timer: one function, and one place that turns a clock difference into milliseconds
    assert [f for f, _ in definitions(r'\bdouble\s+ms_\w+' + body)] == ['zkc_host_util.h']
    assert [f for f, _ in definitions(r'duration\s*<\s*double\s*,\s*std::milli\s*>')] == ['zkc_host_util.h']
    assert [f for f, _ in definitions(r'0xd992f6edu')] == ['zkc_host_util.h']       # first word of the G2 generator
    # the check of the points of a file: one device entry and one host-thread loop, whichever file of kernels asks
    assert [f for f, _ in definitions(r'\bpoints_check_dev' + body)] == ['zkc_fixedbase_dev.hip']
    assert [f for f, _ in definitions(r'\bhost_first_bad' + body)] == ['zkc_file_points.h']
    # body-less declarations of cross-file functions: in headers only
    # a type, then the name, a parameter list and a semicolon (a call has no type in front of it)
    for name in ('zkc_lane_streams', 'zkc_get_template', 'zkc_witness_chunk_async', 'zkc_ctx_lanes_destroy', 'zkc_pairing_bin'):
        decl = re.compile(r'^[ \t]*(?:extern\s+"C"\s+)?(?!return\b|else\b)(?:[A-Za-z_][\w:]*(?:\s*[\*&]+\s*|\s+))+%s\s*\([^;{}]*\)\s*;' % name, re.M)
        assert [f for f, t in text.items() if f.endswith('.hip') and decl.search(t)] == [], name
        assert sum(len(decl.findall(t)) for f, t in text.items() if f.endswith('.h')) <= 1, name
