"""Context: one caller's own fault record, path mode and scratch pool (include/simaps_ctx.h).

Without a context every launch of the process posts into one fault word and obeys one path mode: a
bad descriptor in one collector thread's launch fails whichever call comes next, from any thread
and for any device.  A host that drives several GPUs from one process, or several collectors from
several threads, makes one Context per collector thread (or per device) and passes it as
`context=` to the batch objects (StateBatch, MixedStateBatch, VectorEnvObservations, GridGraph,
OccupancyMap) and the module functions of simaps.batch; their launches then go through the
simaps_ctx_* twins, bit-identical to the plain entry points.

Thread safety: different contexts need no coordination.  One context may be shared by several
threads, which then share its one fault record.  close() (simaps_ctx_destroy) synchronises the
context's device first; it must not run while another thread is inside a call through the context.
"""
import ctypes

import torch

from . import _lib

_FAULT_NAMES = ((_lib.FAULT_TIMEOUT, 'barrier-timeout'), (_lib.FAULT_ROUNDS, 'sssp-round-cap'),
                (_lib.FAULT_DESCRIPTOR, 'descriptor-clamped'))


class Context:
    """A created context on `device` ('cuda' = the current device, or 'cuda:<n>')."""

    def __init__(self, device='cuda', L=None):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise ValueError('a Context lives on a GPU device (got %s); there is no CPU path' % dev)
        self._L = L or _lib.lib
        self.handle, self._open = None, False
        h = ctypes.c_void_p()
        _lib.check(self._L.simaps_ctx_create(-1 if dev.index is None else dev.index, ctypes.byref(h)), self._L)
        self.handle, self._open = h, True
        self.device = torch.device('cuda', self._L.simaps_ctx_device(h))

    def path_mode(self, mode):
        """Set this context's path mode (0-3, simaps_path_mode's values); returns the previous one."""
        prev = self._L.simaps_ctx_path_mode(self.handle, int(mode))
        if prev < 0:
            _lib.check(prev, self._L)
        return prev

    def fault_info(self, clear=False):
        """(bits, kernel name or None, unit or None) of the launches through this context that have
        completed (synchronise the stream first to cover a given launch).  The unit is the index
        along the faulting call's batch dimension: the agent, query or frame."""
        k, u = ctypes.c_int(-1), ctypes.c_int(-1)
        f = self._L.simaps_ctx_fault_info(self.handle, int(bool(clear)), ctypes.byref(k), ctypes.byref(u))
        if f < 0:
            _lib.check(f, self._L)
        if k.value < 0:
            return f, None, None
        return f, _lib.K_NAMES.get(k.value, 'kernel %d' % k.value), u.value

    def fault_status(self, clear=False):
        return self.fault_info(clear)[0]

    def check_faults(self):
        """Raise DeviceFault if a completed launch through this context reported a device-side fault
        (clears the record), naming the kernel and unit when known."""
        f, kernel, unit = self.fault_info(clear=True)
        if f:
            where = '' if kernel is None else ' in %s, unit %d' % (kernel, unit)
            raise _lib.DeviceFault('device fault bits 0x%x (%s)%s: the outputs of a completed launch are invalid' % (
                f, ' '.join(n for b, n in _FAULT_NAMES if f & b), where))

    def close(self):
        """Destroy the context (synchronises its device first).  Idempotent.  The handle is kept: a
        later call through it is refused by the library (SimapsError), not undefined."""
        if self._open:
            self._open = False
            _lib.check(self._L.simaps_ctx_destroy(self.handle), self._L)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # best effort (interpreter shutdown, a device already gone)
            pass


def for_device(context, device):
    """`context` checked against an object's device (None passes): the context the object uses."""
    if context is not None and context.device != device:
        raise ValueError('the context lives on %s, the object on %s' % (context.device, device))
    return context
