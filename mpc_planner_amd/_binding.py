"""The one ctypes binding path of the package: what solver.py (include/tmpc_hip.h) and the stack modules (tmpc_hip_stack*.h) do with a signature
table `name -> (restype, argtypes)` whose first argtype is the handle.  bind() sets the table on a library, converters() derives how every
argument behind the handle is converted, invoke() calls an entry on a handle, check() turns a code into TmpcError.  StackEntries is the base of
StackWriters / StackEnvironment / StackScenario; _column, _cols and _count are what their wrappers share."""
import ctypes as C

_INTEGERS = (C.c_int, C.c_int32, C.c_uint32, C.c_uint64)
_CTYPES = (C._SimpleCData, C.Array, C.Structure, C._Pointer, type(C.byref(C.c_int())))


class TmpcError(RuntimeError):
    pass


def _pointer(v):
    """None or 0: NULL; an integer address as it is; a ctypes object (c_void_p, byref(..), an array) untouched."""
    return v if v is None or isinstance(v, _CTYPES) else int(v) or None


def bind(lib, signatures):
    """restype / argtypes of every entry of the table that the library has.  An older build of the same C-ABI (A/B runs, a library built
    before a header existed) may lack an entry: skipped here, refused when called."""
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes


def converters(signatures):
    """Per entry, how each argument behind the handle is converted: counts through int() and reals through float() (a numpy scalar is a
    TypeError to ctypes otherwise), everything else is a pointer."""
    return {name: tuple(int if t in _INTEGERS else float if t is C.c_double else _pointer for t in argtypes[1:])
            for name, (_, argtypes) in signatures.items()}


def invoke(lib, handle, name, convert, args):
    """The one path into a library: entry `name` on `handle`, every argument converted as convert[name] says; returns the entry's code as it
    is (for the entries whose non-negative return is a value)."""
    fn = getattr(lib, name, None)
    if fn is None:
        raise TmpcError(f"this library has no {name} (a missing kernel is an error, there is no host fallback)")
    return fn(handle, *[c(a) for c, a in zip(convert[name], args)])


def check(lib, handle, rc, what):
    if rc != 0:
        raise TmpcError(f"{what} failed ({rc}): {lib.tmpc_last_error(handle).decode()}")


class StackEntries:
    """The entry points of one stack header -- the subclass's table _SIGNATURES -- on a BatchedSolver's library and handle (raw device
    pointers, like BatchedSolver's own wrappers).  Everything is enqueued on the handle's stream; a failure raises TmpcError with the
    library's message."""
    _SIGNATURES = {}

    def __init_subclass__(cls):
        cls._CONVERT = converters(cls._SIGNATURES)

    def __init__(self, solver):
        self.solver = solver
        bind(solver.lib, self._SIGNATURES)

    def _call(self, name, *args):
        s = self.solver
        check(s.lib, s._h, invoke(s.lib, s._h, name, self._CONVERT, args), name)


def _column(parameter_map, name):
    try:
        return int(parameter_map[name])
    except KeyError:
        raise KeyError(f"the parameter map has no {name!r}: not a stack with these rows") from None


def _cols(cols):
    return None if cols is None else (C.c_int32 * max(len(cols), 1))(*[int(c) for c in cols])


def _count(cols, per, lead=0):
    """The entries (rows, segments) a cols list names: `lead` columns, then `per` per entry."""
    n = len(cols) - lead if cols is not None and len(cols) else 0
    if n % per:
        raise ValueError(f"cols holds {lead} + {per} per entry (an entry per row or segment): its length is not {lead} plus a multiple of {per}")
    return n // per
