"""The boundary is a C ABI: include/ctdet.h must be plain C (no C++ or torch types) and a C program must link
against libctdet.so and get the known answers from the host entry points (no GPU needed)."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, 'context-transformer_amd', 'lib')


@pytest.mark.skipif(shutil.which('gcc') is None, reason='gcc not available')
def test_header_is_c99_and_c_caller_links(tmp_path):
    assert os.path.exists(os.path.join(LIBDIR, 'libctdet.so')), 'build the library first (context-transformer_amd/build.py)'
    exe = str(tmp_path / 'c_caller')
    cmd = ['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I' + os.path.join(REPO, 'include'),
           os.path.join(REPO, 'examples', 'c_caller.c'), '-L' + LIBDIR, '-lctdet', '-Wl,-rpath,' + LIBDIR, '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert 'cpu_nms keeps 2: 0 2' in r.stdout


@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_reference_native_symbol_is_exported_with_cxx_linkage(tmp_path):
    """utils/nms/gpu_nms.hpp:1-2 declares `void _nms(int*, int*, const float*, int, int, float, int)` with C++
    linkage; libctdet exports exactly that symbol, so a translation unit that only knows the reference's prototype
    (examples/cpp_caller.cpp) links against it."""
    r = subprocess.run(['nm', '-D', '--defined-only', os.path.join(LIBDIR, 'libctdet.so')], capture_output=True, text=True)
    assert r.returncode == 0 and ' T _Z4_nmsPiS_PKfiifi' in r.stdout
    exe = str(tmp_path / 'cpp_caller')
    r = subprocess.run(['g++', '-Wall', '-Werror', os.path.join(REPO, 'examples', 'cpp_caller.cpp'), '-L' + LIBDIR, '-lctdet',
                        '-Wl,-rpath,' + LIBDIR, '-Wl,-z,now', '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# The reference's header (utils/nms/gpu_nms.hpp:1-2), i.e. the prototype examples/cpp_caller.cpp declares: a Cython
# module built with `cdef extern from "gpu_nms.hpp"` sees exactly this declaration.
GPU_NMS_HPP = ('void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,\n'
               '          float nms_overlap_thresh, int device_id);\n')

# A Cython binding in the reference's form (a C++ module whose `cdef extern from "gpu_nms.hpp"` block declares `_nms`
# and hands it a contiguous float32 [N, 5] host array), written for this test so that it needs nothing outside the repo.
GPU_NMS_PYX = '''
cdef extern from "gpu_nms.hpp":
    void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
              float nms_overlap_thresh, int device_id)

def gpu_nms(float[:, ::1] sorted_dets, float thresh, int device_id=0):
    """Indices (into sorted_dets, rows in descending score order) that NMS keeps."""
    cdef int n = sorted_dets.shape[0]
    cdef int num_out = 0
    cdef int[::1] keep = memoryview(bytearray(4 * max(n, 1))).cast('i')
    if n:
        _nms(&keep[0], &num_out, &sorted_dets[0, 0], n, sorted_dets.shape[1], thresh, device_id)
    return [keep[i] for i in range(num_out)]
'''


@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_reference_gpu_nms_pyx_links_against_libctdet(tmp_path):
    """A Cython binding of the reference's form (utils/nms/gpu_nms.pyx: `cdef extern from "gpu_nms.hpp"`, `_nms` called on
    a host array) built against libctdet instead of the reference's nvcc object.  Cython emits the call from the header's
    prototype with C++ linkage; the module must link with every symbol bound at load (-z now) and import.  Running it
    needs a GPU and is covered by tests/test_gpu_kernels.py through the same symbol."""
    pytest.importorskip('Cython')
    import sysconfig
    (tmp_path / 'gpu_nms.hpp').write_text(GPU_NMS_HPP)
    pyx = tmp_path / 'gpu_nms.pyx'
    pyx.write_text(GPU_NMS_PYX)
    cpp = str(tmp_path / 'gpu_nms.cpp')
    r = subprocess.run([sys.executable, '-m', 'cython', '--cplus', '-3', str(pyx), '-o', cpp], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert '#include "gpu_nms.hpp"' in open(cpp).read()      # the declaration comes from the header, as in the reference
    so = str(tmp_path / ('gpu_nms' + sysconfig.get_config_var('EXT_SUFFIX')))
    cmd = ['g++', '-shared', '-fPIC', '-O1', '-w', cpp, '-I' + str(tmp_path),
           '-I' + sysconfig.get_paths()['include'], '-L' + LIBDIR, '-lctdet', '-Wl,-rpath,' + LIBDIR, '-Wl,-z,now', '-o', so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(['nm', '-D', '--undefined-only', so], capture_output=True, text=True)
    assert '_Z4_nmsPiS_PKfiifi' in r.stdout                   # the binding really calls the C++-linkage symbol
    # import in a fresh interpreter (torch first: libctdet must bind to torch's HIP runtime, see ctdet/_lib.py)
    code = 'import torch, sys; sys.path.insert(0, %r); import gpu_nms; print(callable(gpu_nms.gpu_nms))' % str(tmp_path)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0 and 'True' in r.stdout, r.stderr[-2000:]
