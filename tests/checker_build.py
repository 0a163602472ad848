"""The one compile-and-load step of the tests' C checkers: tests/<name>.c, each of which includes the oracle unchanged, compiled with the
CFLAGS of oracle/Makefile and loaded with ctypes.  Test infrastructure only."""
import ctypes
import os
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_libs = {}
_tmp = None         # the directory of the builds that were given none; it goes when the interpreter does (a loaded library may be unlinked)


def compile_checker(source_name, directory=None):
    """tests/`source_name` as a loaded library: compiled once per process, into `directory` or into a temporary one"""
    global _tmp
    if source_name not in _libs:
        if directory is None:
            _tmp = _tmp or tempfile.TemporaryDirectory(prefix="checkers_")
            directory = _tmp.name
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        cflags = re.search(r"^CFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()
        so = os.path.join(directory, "lib" + os.path.splitext(source_name)[0] + ".so")
        subprocess.check_call(["gcc", *cflags, "-shared", "-o", so, os.path.join(HERE, source_name), "-lm"])
        _libs[source_name] = ctypes.CDLL(so)
    return _libs[source_name]
