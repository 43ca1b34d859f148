"""What the CPU-side ABI tests (tests/test_*_abi.py) share: a function's parameter list as the header declares it, the kind of ctypes class each parameter
binds to, the kind a class of binding.py's tables is, and a numpy array as a C pointer.  A plain module, like tests/parity.py: no fixtures, no hooks."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decl(name, header="mon_core.h"):
    """the parameter declarations of `int name(...)` in include/<header>, comments removed"""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, "%s is not declared in %s" % (name, header)
    return [a.strip() for a in m.group(1).split(",")]


def kind(arg):
    """the kind of ctypes class a C parameter declaration binds to in binding.py's tables (size_t and uint64_t are one ctypes class on LP64)"""
    if "*" in arg:
        return "ptr"
    return {"size_t": "u64", "int": "int", "uint32_t": "uint32", "uint64_t": "u64", "float": "float"}[arg.split()[1 if arg.startswith("const") else 0]]


def bound(t):
    """the kind of a ctypes class of binding.py's tables"""
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)):
        return "ptr"
    return {C.c_size_t: "u64", C.c_uint64: "u64", C.c_int: "int", C.c_uint32: "uint32", C.c_float: "float"}[t]


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)
