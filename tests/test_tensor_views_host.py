"""The tensor records and channel-slice views of the engine's host code (csrc/tensor_views.h), checked on the host: no GPU.

tests/host/tensor_views_main.cpp includes only that header; it is built here with AddressSanitizer and UBSan as an ordinary
executable and prints what a view derives from its tensor and how a TensorSet hands out absmax slots.  Checked against the
formulas the engine used while a slice travelled as (pointer, pitch, pointer of the tensor it is a view of), written out
below: for a slice y of the tensor at ykey with pitch ldy that holds `cout` channels
    mask bytes   m8(ykey) + (y - ykey) / 4, pitch ldy / 4
    pair sibling p + (y - ykey) * 4
    whole tensor ldy == cout
and slot indices in first-use order (the size of the per-phase registry at first use), none past 384 per phase, a new
phase clearing every `valid` flag of that phase and no index."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSLOTS = 384
N = 400
# (tensor width, first channel, channels)
SLICES = ([(304, 0, 256), (304, 256, 48), (304, 0, 304)] + [(1280, 256 * i, 256) for i in range(4)] +
          [(1280, 1024, 256), (1280, 0, 1280)])


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('tensor_views') / 'tensor_views_main')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tests', 'host', 'tensor_views_main.cpp'), '-o', exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    return [line.split() for line in p.stdout.splitlines()]


def test_a_view_derives_its_pointers_by_the_engines_formulas(printed):
    rows = {}
    for w in printed:
        if w[0] == 'view':
            rows.setdefault(tuple(int(v) for v in w[1:4]), {}).update(zip(w[4::2], (int(v) for v in w[5::2])))
    assert sorted(rows) == sorted(SLICES)
    for (ld, c0, c), r in rows.items():
        off = c0                                   # y - ykey, in floats
        assert (r['data'], r['ld']) == (off, ld)
        assert (r['mask'], r['ldmask']) == (off // 4, ld // 4)
        assert r['sibling'] == off * 4
        assert r['whole'] == int(ld == c) and (r['whole'] == 0 or c0 == 0)
        # no mask bytes: none to read or write; a frozen tensor's bytes are read but not written
        assert r['nomask'] == 1 and r['towrite'] == r['mask'] and r['frozen_towrite_null'] == 1 and r['frozen_read'] == r['mask']
    assert sorted(tuple(int(v) for v in w[1:]) for w in printed if w[0] == 'whole_ctor') == [(304, 0, 304, 1), (1280, 0, 1280, 1)]
    assert [w[1:] for w in printed if w[0] == 'none'] == [['1', '0']]


def test_slots_go_out_in_first_use_order_up_to_the_cap(printed):
    use = [(int(w[1]), int(w[2]), int(w[3])) for w in printed if w[0] == 'use']
    assert len(use) == 2 * N
    registry = ({}, {})                            # per phase: tensor -> index, as the pointer-keyed map assigned them
    for ph, i, got in use:
        reg = registry[ph]
        if i not in reg and len(reg) < TSLOTS:
            reg[i] = len(reg)
        assert got == reg.get(i, -1), (ph, i)
    for reg in registry:
        assert sorted(reg.values()) == list(range(TSLOTS))         # the 385th tensor of a phase got none ...
    again = {(int(w[1]), int(w[2])): int(w[3]) for w in printed if w[0] == 'again'}
    assert len(again) == 2 * N
    for (ph, i), got in again.items():                             # ... and asking again changes nothing for anyone
        assert got == registry[ph].get(i, -1), (ph, i)


def test_a_new_phase_clears_the_valid_flags_and_keeps_the_indices(printed):
    again = {(int(w[1]), int(w[2])): int(w[3]) for w in printed if w[0] == 'again'}
    after0 = {(int(w[1]), int(w[2])): (int(w[3]), int(w[4])) for w in printed if w[0] == 'newphase0'}
    after1 = {(int(w[1]), int(w[2])): (int(w[3]), int(w[4])) for w in printed if w[0] == 'newphase1'}
    assert len(after0) == 2 * N and len(after1) == N
    for (ph, i), (slot, valid) in after0.items():
        assert slot == again[ph, i]
        assert valid == (0 if ph == 0 else int(slot >= 0)), (ph, i)       # the other phase keeps its flags
    for (ph, i), (slot, valid) in after1.items():
        assert slot == again[ph, i] and valid == 0


def test_records_do_not_move(printed):
    assert [w[1] for w in printed if w[0] == 'stable'] == ['1']
