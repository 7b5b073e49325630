"""What the ABI tests (test_*_abi.py) share (no tests in here): where the header is and what it says, the C99 compile of a
caller, and the scaffolding of the refusal tests -- a handle that is never dereferenced, what an output handle holds
before the call, the library's last message, an out-struct filled with a byte and the check that a refusal zeroed it.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import bspgemm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bspgemm.h")
ERR_INVALID = 1
FAKE = C.c_void_p(64)          # never dereferenced: a refusal comes before the operand is looked at
SENTINEL = 0x5A5A5A5A          # what every output handle holds before the call: a refused call must have made it NULL


@functools.lru_cache(maxsize=None)
def header_text():
    """include/bspgemm.h as it stands"""
    return open(HEADER).read()


@functools.lru_cache(maxsize=None)
def header_code():
    """the header with every comment replaced by a space and every run of whitespace by one space"""
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S))


def compile_c99(tmp_path, source):
    """`source` as tmp_path/caller.c against the header, strict C99 with every warning an error: the completed process"""
    src = tmp_path / "caller.c"
    src.write_text(source)
    return subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "caller.o")], capture_output=True, text=True)


def last_error():
    return bspgemm.lib().bspgemm_last_error().decode(errors="replace")


def dirtied(struct_type, byte):
    """an out-struct of `byte` bytes: a refused or failed call must have zeroed it"""
    s = struct_type()
    C.memset(C.byref(s), byte, C.sizeof(s))
    return s


def is_zeroed(info):
    return bytes(info) == bytes(C.sizeof(info))
