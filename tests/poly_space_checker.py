"""ctypes binding of tests/cpp/poly_space_checker.cpp: the CPU checker of tests/poly_checker.py plus what its search keeps per node
and does not hand out -- the predecessor lists -- and bulk dumps of the nodes and of the blocked primitives of the closed ones.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from tests import poly_checker

ROOT = poly_checker.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "poly_space_checker.cpp")


_lib = None


def lib():
    """The checker library with the exports of poly_space_checker.cpp: the pc_* entry points of tests/poly_checker.py (declared by its
    own lib(), pointed at this source for the one call) plus psc_*.  tests/poly_checker.py keeps the library it has."""
    global _lib
    if _lib is not None:
        return _lib
    saved = poly_checker._lib, poly_checker.SRC
    try:
        poly_checker._lib, poly_checker.SRC = None, SRC
        L = poly_checker.lib()
    finally:
        poly_checker._lib, poly_checker.SRC = saved
    P, I, V, LL = C.c_void_p, C.c_int, C.c_void_p, C.c_longlong
    L.psc_pred_len.argtypes = [P, I]
    L.psc_pred_get.argtypes = [P, I, V, V]
    L.psc_pred_all.argtypes = [P, LL, V, V, V]
    L.psc_pred_all.restype = LL
    L.psc_nodes_all.argtypes = [P, V, V, V, V, V]
    L.psc_blocked_all.argtypes = [P, LL, V, V]
    L.psc_blocked_all.restype = LL
    _lib = L
    return L


class SpaceChecker(poly_checker.CheckerWorld):
    """CheckerWorld whose last plan's state space can be read out whole."""

    def __init__(self, *a, **kw):
        saved = poly_checker._lib
        poly_checker._lib = lib()
        try:
            super().__init__(*a, **kw)
        finally:
            poly_checker._lib = saved

    def pred(self, i):
        """(parent, action) records of node i, oldest first"""
        n = self.L.psc_pred_len(self.h, int(i))
        p = np.zeros(max(n, 1), dtype=np.int32); a = p.copy()
        self.L.psc_pred_get(self.h, int(i), p.ctypes.data, a.ctypes.data)
        return p[:n], a[:n]

    def space(self):
        """dict like PolyTeam.state_space(): states n x 9 at Dim 2, g, h, closed, opened, child, parent, action"""
        n = self.L.pc_num_nodes(self.h)
        states = np.zeros((max(n, 1), self.ns)); g = np.zeros(max(n, 1)); h = g.copy()
        closed = np.zeros(max(n, 1), dtype=np.int32); opened = closed.copy()
        if n:
            self.L.psc_nodes_all(self.h, states.ctypes.data, g.ctypes.data, h.ctypes.data, closed.ctypes.data, opened.ctypes.data)
        m = int(self.L.psc_pred_all(self.h, 0, None, None, None))
        child = np.zeros(max(m, 1), dtype=np.int32); parent = child.copy(); action = child.copy()
        self.L.psc_pred_all(self.h, m, child.ctypes.data, parent.ctypes.data, action.ctypes.data)
        return dict(n_nodes=n, states=states[:n], g=g[:n], h=h[:n], closed=closed[:n], opened=opened[:n], child=child[:m], parent=parent[:m],
                    action=action[:m])

    def blocked(self):
        """(parent, action) of the blocked primitives: closed nodes in id order, the actions for which get_succ(node state) returns +inf"""
        m = int(self.L.psc_blocked_all(self.h, 0, None, None))
        p = np.zeros(max(m, 1), dtype=np.int32); a = p.copy()
        self.L.psc_blocked_all(self.h, m, p.ctypes.data, a.ctypes.data)
        return p[:m], a[:m]
