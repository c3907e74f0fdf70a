"""CPU: _lib.call, the one way kernels are launched from Python -- what it does with its arguments (against a stub
library: no GPU, no built library needed), and two static checks over the sources: every call site names a bound entry
point with the header's number of arguments, and nothing in the package reaches an entry point any other way."""
import ast
import ctypes
import gc
import glob
import importlib
import os
import weakref

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = importlib.import_module("3dod_amd._lib")


class _StubLib:
    """stands in for the loaded library: cr_<anything>(ctx, *args) records its arguments, runs `during` and returns `rc`"""

    def __init__(self, rc=0, during=None):
        self.rc, self.during, self.calls = rc, during, []

    def cr_last_error(self):
        return b"stub says no"

    def __getattr__(self, name):
        if not name.startswith("cr_"):
            raise AttributeError(name)

        def fn(ctx, *args):
            self.calls.append((name, ctx, args))
            if self.during is not None:
                self.during(args)
            return self.rc
        return fn


@pytest.fixture
def stub(monkeypatch):
    s = _StubLib()
    monkeypatch.setattr(_lib, "load", lambda: s)
    monkeypatch.setattr(_lib, "ctx_for", lambda device: ("ctx", str(device)))
    return s


def test_call_keeps_its_tensor_arguments_alive_until_the_entry_point_returns(stub):
    """the property hipops._Args existed for: an inline temporary (the only reference is the argument itself) is alive,
    at the address that was passed, while the C function runs, and is released when call returns"""
    t = torch.arange(64, dtype=torch.float32)
    ref, addr = weakref.ref(t), t.data_ptr()
    holder = [t]
    del t
    seen = {}

    def during(args):
        gc.collect()
        seen["alive"] = ref() is not None
        seen["ptr"] = args[0].value
        seen["addr_now"] = ref().data_ptr() if ref() is not None else None
    stub.during = during
    _lib.call("cr_gelu_inplace", holder.pop(), 64)
    assert seen["alive"], "call let go of a tensor argument before the entry point ran"
    assert seen["ptr"] == addr == seen["addr_now"]
    gc.collect()
    assert ref() is None, "call kept a tensor argument after it returned"


def test_call_argument_conversion_and_errors(stub):
    x = torch.zeros(4, 6)
    arr = (ctypes.c_int * 3)(1, 2, 3)
    cast = ctypes.cast(arr, ctypes.c_void_p)
    _lib.call("cr_layernorm", x, None, arr, cast, 7, 0.5)
    (name, ctx, args), = stub.calls
    assert name == "cr_layernorm" and ctx == ("ctx", "cpu")                   # the context of the first tensor argument
    assert isinstance(args[0], ctypes.c_void_p) and args[0].value == x.data_ptr()
    assert isinstance(args[1], ctypes.c_void_p) and args[1].value is None      # None -> NULL
    assert args[2] is arr and args[3] is cast and args[4] == 7 and type(args[4]) is int and args[5] == 0.5
    # device= gives the context when no argument is a tensor; without either there is nothing to launch on
    _lib.call("cr_conv2d_fwd_group", 2, cast, device=torch.device("cpu"))
    assert stub.calls[-1][1] == ("ctx", "cpu")
    with pytest.raises(_lib.CrError):
        _lib.call("cr_conv2d_fwd_group", 2, cast)
    n = len(stub.calls)
    with pytest.raises(_lib.CrError, match="dense"):
        _lib.call("cr_gelu_inplace", x.t(), 24)                                # a non-dense tensor
    with pytest.raises(_lib.CrError, match="cr_no_such_kernel"):
        _lib.call("cr_no_such_kernel", x)                                      # not in SIGNATURES
    assert len(stub.calls) == n, "an entry point ran although call had to refuse"
    stub.rc = 3
    with pytest.raises(_lib.CrError) as e:
        _lib.call("cr_gelu_inplace", x, 24)
    assert "cr_gelu_inplace" in str(e.value) and "stub says no" in str(e.value) and "rc=3" in str(e.value)


def test_call_has_no_cpu_path(monkeypatch):
    """with the real ctx_for a CPU tensor is refused before the entry point runs"""
    s = _StubLib()
    monkeypatch.setattr(_lib, "load", lambda: s)
    with pytest.raises(_lib.CrError, match="no CPU path"):
        _lib.call("cr_gelu_inplace", torch.zeros(8), 8)
    assert not s.calls


# ---- static checks ----------------------------------------------------------------------------------------------------------
def _sources():
    files = glob.glob(os.path.join(ROOT, "3dod_amd", "**", "*.py"), recursive=True)
    for d in ("tests", "scripts"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    files = sorted(f for f in files if os.path.abspath(f) != os.path.abspath(__file__))
    assert len(files) > 20
    return files


def _lib_aliases(tree):
    """names bound to the _lib module in a file (`from . import _lib`, `X = importlib.import_module("3dod_amd._lib")`) and
    names bound to its call function (`from ._lib import call`)"""
    mods, funcs = set(), set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            for a in node.names:
                if a.name == "_lib":
                    mods.add(a.asname or a.name)
                if (node.module or "").endswith("_lib") and a.name == "call":
                    funcs.add(a.asname or a.name)
        elif isinstance(node, ast.Import):
            for a in node.names:
                if a.name.endswith("._lib") and a.asname:
                    mods.add(a.asname)
        elif isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) and node.value.args:
            a0 = node.value.args[0]
            if isinstance(a0, ast.Constant) and isinstance(a0.value, str) and a0.value.endswith("._lib"):
                mods.update(t.id for t in node.targets if isinstance(t, ast.Name))
    return mods, funcs


def _call_sites():
    """(file, line, [name literals], number of written-out positional arguments, has a *-expansion) of every _lib.call"""
    sites = []
    for path in _sources():
        tree = ast.parse(open(path).read(), path)
        mods, funcs = _lib_aliases(tree)
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            f = node.func
            if not ((isinstance(f, ast.Attribute) and f.attr == "call" and isinstance(f.value, ast.Name) and f.value.id in mods)
                    or (isinstance(f, ast.Name) and f.id in funcs)):
                continue
            where = f"{os.path.relpath(path, ROOT)}:{node.lineno}"
            assert node.args and not isinstance(node.args[0], ast.Starred), f"{where}: _lib.call without a name"
            first = node.args[0]
            # the name is a string literal, or a choice between string literals (each one is checked)
            lits = [first.body, first.orelse] if isinstance(first, ast.IfExp) else [first]
            assert all(isinstance(c, ast.Constant) and isinstance(c.value, str) for c in lits), \
                f"{where}: the first argument of _lib.call must be a string literal"
            rest = node.args[1:]
            starred = any(isinstance(a, ast.Starred) for a in rest)
            sites.append((where, [c.value for c in lits], sum(not isinstance(a, ast.Starred) for a in rest), starred))
    return sites


# the call sites whose argument list expands a tuple: their arity is only bounded from above.  No new one may appear.
MAX_STARRED_SITES = 3


def test_every_call_site_names_an_entry_point_with_the_headers_arity():
    sites = _call_sites()
    exact = weak = 0
    for where, names, nargs, starred in sites:
        for name in names:
            assert name in _lib.SIGNATURES, f"{where}: {name} is not in SIGNATURES"
            sig = _lib.SIGNATURES[name]
            assert sig and sig[0] is _lib.P and name not in ("cr_ctx_destroy", "cr_ctx_set_stream"), \
                f"{where}: {name} takes no context / returns no status: not for _lib.call"
            want = len(sig) - 1
            if starred:
                assert nargs <= want, f"{where}: {name} takes {want} arguments after the context, {nargs} written out"
            else:
                assert nargs == want, f"{where}: {name} takes {want} arguments after the context, got {nargs}"
        weak += starred
        exact += not starred
    print(f"_lib.call sites: {exact} checked exactly, {weak} with a *-expansion (upper bound only)")
    assert exact >= 100, "the scan does not see the call sites any more"
    assert weak <= MAX_STARRED_SITES


def test_no_entry_point_is_reached_outside_lib():
    """outside _lib.py no attribute whose name starts with cr_ is read from any object in the package"""
    bad = []
    for path in glob.glob(os.path.join(ROOT, "3dod_amd", "**", "*.py"), recursive=True):
        if os.path.basename(path) == "_lib.py":
            continue
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.Attribute) and node.attr.startswith("cr_"):
                bad.append(f"{os.path.relpath(path, ROOT)}:{node.lineno}: .{node.attr}")
    assert not bad, "entry points are called through _lib.call only:\n" + "\n".join(bad)
