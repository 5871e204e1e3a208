"""Every public header (include/bsig*.h) against the binding's table of its prototypes (_lib.HEADERS): the names
the header declares are the names of its table, the built library exports each, no name belongs to two headers,
and no header is without a table or table without a header.  What is particular to one header (the ``_f64`` and
``_ex`` prototypes, its constants, the routing of the precision seam) is asserted next to that feature's tests."""
import ctypes
import glob
import os
import re

import pytest

from conftest import ROOT

from bayes_sim_ig_amd import _lib

INCLUDE = os.path.join(ROOT, 'include')


def _declared(header):
    with open(os.path.join(INCLUDE, header)) as f:
        text = f.read()
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)      # a comment may name another header's function
    return set(re.findall(r'\b(bsig_[a-z0-9_]+)\s*\(', text))


def test_every_header_has_a_table_and_every_table_a_header():
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, '*.h')))
    assert on_disk == sorted(_lib.HEADERS) and 'bsig.h' in on_disk
    assert on_disk == sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, 'bsig*.h')))
    assert _lib.exported_symbols() == _lib.exported_symbols('bsig.h')
    everything = _lib.exported_symbols(None)
    assert everything == sorted(_lib.PROTOS) == sorted(n for h in _lib.HEADERS for n in _lib.exported_symbols(h))
    assert len(everything) == len(set(everything))


@pytest.mark.parametrize('header', sorted(_lib.HEADERS))
def test_header_matches_binding(header):
    declared = _declared(header)
    assert declared and declared == set(_lib.exported_symbols(header)) == set(_lib.HEADERS[header])
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name in sorted(declared):
        assert hasattr(raw, name), name
        res, args = _lib.HEADERS[header][name]
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for other in _lib.HEADERS:
        if other != header:
            assert not declared & set(_lib.exported_symbols(other)), other
            assert not declared & _declared(other), other
    assert bound.bsig_version() >= 100


def test_a_name_in_two_headers_fails_the_import():
    assert _lib._merged(_lib.HEADERS) == _lib.PROTOS
    twice = dict(_lib.HEADERS, **{'bsig_next.h': {'bsig_version': (ctypes.c_int, [])}})
    with pytest.raises(ImportError, match='bsig_next.h.*bsig_version'):
        _lib._merged(twice)
