"""CPU: the one owner of a library handle in libfsm_amd/capi.py (_Owned) and the classes that derive from it.  No library call:
the objects are made with __new__ and a stub in _lib that counts the calls of every function."""
import ctypes as C
import gc

import pytest

from libfsm_amd import capi
from libfsm_amd.capi import _Freed, _Owned

OWNERS = ["Plan", "HipDfa", "HipNode", "MultiPrepared", "LinesDfa", "HipText", "HipHits", "PosDfa", "HipSpans", "TokDfa", "HipTokens",
          "HipMatches", "HipRepl", "HipReplaced", "HipRules", "HipExtracted", "HipDistinct"]
FREED = OWNERS[-6:]             # close() is spelt free() as well, as before; no other class has a free()


class Stub:
    """stands in for the loaded library: every attribute is a function that records (name, argument)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name,) + args)


def made(cls, handle=0x1000, keep=("kept",)):
    obj = cls.__new__(cls)
    obj._lib, obj._h, obj._keep = Stub(), handle, keep
    return obj


def subclasses(cls):
    for sub in cls.__subclasses__():
        yield sub
        yield from subclasses(sub)


def test_the_seventeen_classes_and_no_other_derive_from_the_owner():
    assert sorted(c.__name__ for c in subclasses(_Owned) if c is not _Freed) == sorted(OWNERS)
    assert sorted(c.__name__ for c in subclasses(_Freed)) == sorted(FREED)
    assert [name for name in OWNERS if hasattr(getattr(capi, name), "free")] == FREED
    assert all(getattr(capi, name).__module__ == capi.__name__ for name in OWNERS)


@pytest.mark.parametrize("name", OWNERS)
def test_free_function_is_in_the_prototype_table(name):
    """_FREE names a function of PROTOTYPES that returns nothing and takes one pointer"""
    cls = getattr(capi, name)
    assert isinstance(cls._FREE, str) and cls._FREE.startswith("fsm_hip_") and cls._FREE.endswith("_free")
    assert capi.PROTOTYPES[cls._FREE] == (None, [C.c_void_p])


@pytest.mark.parametrize("name", OWNERS)
def test_no_class_aliases_the_finaliser(name):
    """__del__ is the base's, which calls self.close(): an alias written in a class would pass an override by"""
    cls = getattr(capi, name)
    assert "__del__" not in vars(cls) and cls.__del__ is _Owned.__del__
    assert isinstance(vars(_Owned)["handle"], property) and "handle" not in vars(cls)
    assert callable(cls.close) and "free" not in vars(cls)


@pytest.mark.parametrize("name", OWNERS)
def test_close_frees_exactly_once(name):
    cls = getattr(capi, name)
    obj = made(cls)
    if name == "LinesDfa":
        obj.inner = made(capi.HipDfa, 0x2000)
        obj.inner._borrowed = True
    lib = obj._lib
    assert obj.handle == 0x1000
    obj.close()
    assert lib.calls == [(cls._FREE, 0x1000)]
    assert obj._h is None and obj._keep is None and obj.handle is None
    obj.close()
    if name in FREED:
        obj.free()
    obj.__del__()
    assert lib.calls == [(cls._FREE, 0x1000)]


@pytest.mark.parametrize("name", FREED)
def test_free_reaches_the_same_close(name):
    cls = getattr(capi, name)
    obj = made(cls)
    lib = obj._lib
    obj.free()
    assert lib.calls == [(cls._FREE, 0x1000)] and obj._h is None and obj._keep is None

    class Loud(cls):
        closed = 0

        def close(self):
            Loud.closed += 1
            super().close()

    obj = made(Loud)
    obj.free()
    assert Loud.closed == 1 and obj._lib.calls == [(cls._FREE, 0x1000)]


@pytest.mark.parametrize("name", OWNERS)
def test_close_on_a_half_constructed_object_does_nothing(name):
    """__init__ raised before there was a handle: no _h, no _keep, perhaps no _lib"""
    cls = getattr(capi, name)
    obj = cls.__new__(cls)
    obj.close()
    obj.__del__()
    obj = cls.__new__(cls)
    obj._lib = lib = Stub()
    obj.close()
    assert lib.calls == [] and obj._h is None and obj._keep is None
    obj = made(cls, handle=None)
    obj.close()
    assert obj._lib.calls == []


def test_a_borrowed_dfa_never_calls_free():
    dfa = made(capi.HipDfa)
    dfa._borrowed = True
    lib = dfa._lib
    dfa.close()
    dfa.__del__()
    assert lib.calls == [] and dfa._h is None and dfa._keep is None
    owned = made(capi.HipDfa)
    owned._borrowed = False
    owned.close()
    assert owned._lib.calls == [("fsm_hip_dfa_free", 0x1000)]


def test_the_finaliser_reaches_an_overridden_close():
    """LinesDfa.close clears the borrowed inner handle before the twin is freed; dropping the last reference runs it"""
    ld = made(capi.LinesDfa)
    inner = ld.inner = made(capi.HipDfa, 0x2000)
    inner._borrowed = True
    lib = ld._lib
    del ld
    gc.collect()
    assert inner._h is None and inner._lib.calls == []
    assert lib.calls == [("fsm_hip_lines_dfa_free", 0x1000)]

    class Loud(capi.HipTokens):
        closed = 0

        def close(self):
            Loud.closed += 1
            super().close()

    t = made(Loud)
    lib = t._lib
    del t
    gc.collect()
    assert Loud.closed == 1 and lib.calls == [("fsm_hip_tokens_free", 0x1000)]


def test_hits_let_go_of_their_text():
    hits = made(capi.HipHits)
    hits._text = object()
    hits.close()
    assert hits._text is None and hits._keep is None


def test_a_template_table_is_fully_initialised(monkeypatch):
    """HipRepl.template builds its object without HipRepl.__init__: it still has its library, its handle and its counts"""
    lib = Stub()
    monkeypatch.setattr(capi, "load_library", lambda: lib)
    monkeypatch.setattr(capi, "_call", lambda name, *args: 0x3000)
    rp = capi.HipRepl.template([b"<>", b""], [[1], []], capi.REPL_MASK)
    assert rp._lib is lib and rp.handle == 0x3000 and rp._keep == () and (rp.nrepl, rp.flags) == (2, capi.REPL_MASK)
    plain = capi.HipRepl([b"a"])
    assert plain._lib is lib and plain.handle == 0x3000 and plain._keep == () and (plain.nrepl, plain.flags) == (1, 0)
    rp.close()
    plain.free()
    assert lib.calls == [("fsm_hip_repl_free", 0x3000)] * 2
