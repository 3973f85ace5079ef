"""Resource limits that let the teacher-forced decoder attention share a CU with a resident lstm_tile_kernel
workgroup (64 KB of LDS, 8 waves, 96 VGPRs; a CU has 160 KB and 512 VGPRs per SIMD), checked on the compiler's own
figures -- no GPU needed.  csrc/kernels_seq2seq.hip is compiled for gfx950 to assembly and the code-object metadata
of dec_attn_ring_kernel<2> is read: at most 512 threads, at most 104 VGPRs, no scratch.  Its dynamic LDS request at
T_enc 45 and 20 decoder steps, at most 48 KB, is the launcher's own figure (n2nmn_debug_dec_attn;
kernels_seq2seq.hip also asserts it at compile time).
"""
import ctypes
import os
import re
import subprocess

import pytest

from n2nmn_amd import _lib, build

CSRC = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), 'csrc')


@pytest.fixture(scope='module')
def kernel_metadata(tmp_path_factory):
    """{kernel symbol: {metadata key: int}} of csrc/kernels_seq2seq.hip compiled as the library compiles it"""
    out = str(tmp_path_factory.mktemp('ring') / 'kernels_seq2seq.s')
    cmd = [build.hipcc(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '-fPIC', '-x', 'hip',
           '--cuda-device-only', '-S', os.path.join(CSRC, 'kernels_seq2seq.hip'), '-o', out]
    subprocess.check_call(cmd)
    text = open(out).read()
    meta = {}
    # one YAML list item per kernel in the amdhsa.kernels note; the keys below are scalars of that item
    for item in re.split(r'\n\s*- \.agpr_count:', text.split('amdhsa.kernels:')[1])[1:]:
        name = re.search(r'\n    \.name:\s+(\S+)', item).group(1)     # (four spaces: the kernel's own, not an argument's)
        meta[name] = {k: int(re.search(r'\n    \.%s:\s+(\d+)' % k, item).group(1)) for k in
                      ('vgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size',
                       'max_flat_workgroup_size')}
    return meta


def _one(meta, pattern):
    hits = [v for k, v in meta.items() if re.search(pattern, k)]
    assert len(hits) == 1, (pattern, [k for k in meta if re.search(pattern, k)])
    return hits[0]


def test_ring_attention_kernel_fits_beside_a_tile_workgroup(kernel_metadata):
    m = _one(kernel_metadata, r'dec_attn_ring_kernelILi2E')
    print('dec_attn_ring_kernel<2>:', m)
    assert m['max_flat_workgroup_size'] <= 512
    assert m['vgpr_count'] <= 104
    assert m['private_segment_fixed_size'] == 0, 'the kernel spills to scratch'
    assert m['group_segment_fixed_size'] == 0          # all of its LDS is the launcher's dynamic request


def test_ring_attention_lds_request_at_the_benchmark_shape():
    L = _lib.lib()
    fn = L.n2nmn_debug_dec_attn
    out = (ctypes.c_uint64 * 4)()
    assert fn(None, out) == 0
    print('dec_attn_ring_kernel: %d B of dynamic LDS at T_enc 45, 20 steps; %d threads' % (out[2], out[3]))
    assert out[2] <= 48 * 1024
    assert out[3] <= 512
