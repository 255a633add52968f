"""The host records of ``ppq_amd/ffi/abi.py`` against the structs of include/ppq_hip.h, as the host compiler lays them out.

One C translation unit is generated from the registry: for every registered struct and every field of its record it prints
``sizeof(struct)``, ``offsetof(struct, field)`` and the field's size.  A field the header does not have does not compile; a struct of
the header that the registry does not name fails the coverage test.  Nothing here needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from ppq_amd import _lib
from ppq_amd.ffi import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ppq_hip.h')
PROF_FIELDS = [name for name, _ in _lib.ProfEntry._fields_]


def _compiler():
    """The first of ``cc`` and hipcc's host pass; a machine that built the library has the second."""
    if shutil.which('cc'): return ['cc', '-x', 'c']
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'no host compiler: neither cc nor hipcc was found'
    return [hipcc, '-x', 'c++', '--offload-host-only']


def _source(layouts) -> str:
    lines = ['#include "ppq_hip.h"', '#include <stddef.h>', '#ifdef __cplusplus', 'extern "C"', '#endif',
             'int printf(const char*, ...);', 'int main(void) {']
    for struct, fields in layouts.items():
        lines.append(f'    printf("{struct} . %zu 0\\n", sizeof({struct}));')
        for field in fields:
            lines.append(f'    printf("{struct} {field} %zu %zu\\n", offsetof({struct}, {field}), sizeof((({struct}*)0)->{field}));')
    return '\n'.join(lines + ['    return 0;', '}', ''])


@pytest.fixture(scope='module')
def compiled(tmp_path_factory):
    """{struct: {field: (offset, size)}} with the struct's own size under '.', as the compiler sees the header."""
    tmp = tmp_path_factory.mktemp('abi_layout')
    layouts = {struct: list(record.names) for struct, record in abi.JOB_LAYOUTS.items()}
    layouts['ppqhip_prof_entry'] = PROF_FIELDS
    src, exe = tmp / 'layout.c', tmp / 'layout'
    src.write_text(_source(layouts))
    build = subprocess.run(_compiler() + ['-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    seen = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        struct, field, first, second = line.split()
        seen.setdefault(struct, {})[field] = (int(first), int(second))
    return seen


def test_the_registry_covers_every_struct_of_the_header():
    named = set(re.findall(r'typedef struct (ppqhip_\w+)', open(HEADER).read()))
    assert named == set(abi.JOB_LAYOUTS), (sorted(named - set(abi.JOB_LAYOUTS)), sorted(set(abi.JOB_LAYOUTS) - named))
    assert len(named) == 28


@pytest.mark.parametrize('struct', sorted(abi.JOB_LAYOUTS))
def test_record_layout_equals_the_struct(compiled, struct):
    record, seen = abi.JOB_LAYOUTS[struct], compiled[struct]
    assert seen['.'][0] == record.itemsize, struct
    assert [name for name in seen if name != '.'] == list(record.names)
    for name in record.names:
        field, offset = record.fields[name][:2]
        assert seen[name] == (offset, field.itemsize), (struct, name)


def test_prof_entry_layout_equals_the_struct(compiled):
    seen = compiled['ppqhip_prof_entry']
    assert seen['.'][0] == ctypes.sizeof(_lib.ProfEntry)
    for name in PROF_FIELDS:
        field = getattr(_lib.ProfEntry, name)
        assert seen[name] == (field.offset, field.size), name
