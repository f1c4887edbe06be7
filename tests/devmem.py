"""Device buffers for tests that drive the raw-pointer entry points without torch: dfx_device_malloc / dfx_memcpy_* of the
handle under test (include/dfx.h), NumPy on the host side."""
import ctypes as C

import numpy as np


class DevBuf:
    """`nbytes` of device memory of FlowEngine `eng`, optionally initialised from a host array; freed by close() or at the
    end of a `with`.  ptr(offset) is the raw pointer `offset` bytes in."""

    def __init__(self, eng, nbytes=None, init=None):
        self.eng = eng
        if init is not None:
            init = np.ascontiguousarray(init)
            nbytes = init.nbytes
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        eng._check(eng._L.dfx_device_malloc(eng._h, C.byref(p), max(self.nbytes, 1)))
        self._p = p
        if init is not None and self.nbytes:
            eng._check(eng._L.dfx_memcpy_h2d(eng._h, p, init.ctypes.data, self.nbytes))

    def ptr(self, offset=0):
        return self._p.value + int(offset)

    def get(self, dtype=np.uint8):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        if self.nbytes:
            self.eng._check(self.eng._L.dfx_memcpy_d2h(self.eng._h, out.ctypes.data, self._p, self.nbytes))
        return out

    def close(self):
        if self._p is not None:
            self.eng._L.dfx_device_free(self.eng._h, self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
