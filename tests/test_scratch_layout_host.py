"""The scratch layouts of the evaluation-stage entry points (csrc/scratch_layout.h), checked on the host: no GPU.

tests/host/scratch_layout_main.cpp includes only that header; it is built here with AddressSanitizer and UBSan as an ordinary
executable and prints, per stage and geometry, every region's offset, size and element size, the arena size `need` and the
range the stage clears.  Checked: regions in bounds, pairwise disjoint, aligned to their element; the cleared range covers
exactly the regions the entry point has always cleared; `need` equals the formula each entry point used before the layouts
existed, written out below (so the library's 512 MB cap rejects at the same frame counts); and the chunk every Python module
computes with its own copy of the formula (`frames_per_call`) stays under that cap."""
import os
import shutil
import subprocess

import pytest

from eosvos_amd import adapt, components, crf, holes, motion, snap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 512 << 20


def pad4(x):
    return (x + 3) // 4 * 4


def pad8(x):
    return (x + 7) // 8 * 8


def clusters(h, w, step):
    return -(-h // step) * -(-w // step)


def davis_need(n, h, w, n_obj):
    map_words = n_obj * h * ((w + 63) // 64)
    chunk = max(1, min((64 << 20) // (2 * map_words * 8), n, 65535))
    return n * n_obj * 6 * 8 + 2 * chunk * map_words * 8


# stage -> need(n, h, w, n_obj, step, erode) as the entry point computed it before the layouts existed (np = n * h * w,
# nk = n * clusters)
NEED = {
    'label_components': lambda n, h, w, o, s, e: pad4(8 * n * h * w),
    'filter_components': lambda n, h, w, o, s, e: pad4(17 * n * h * w + 2312 * n + 256),
    'fill_holes': lambda n, h, w, o, s, e: pad8(4 * (6 * n * h * w + 256 * n)) + 8 * n + 256 * (n + 1),
    'superpixels': lambda n, h, w, o, s, e: 44 * n * clusters(h, w, s),
    'snap_labels': lambda n, h, w, o, s, e: pad8(4 * (n * h * w + (12 + o) * n * clusters(h, w, s))) + 8 * n,
    'block_motion': lambda n, h, w, o, s, e: (n + 1) * h * pad4(w),
    'crf_labels': lambda n, h, w, o, s, e: 12 * (o + 1) * n * h * w,
    'distance_sq': lambda n, h, w, o, s, e: pad4(2 * n * h * w),
    'adapt_targets': lambda n, h, w, o, s, e: pad4(8 * n + 2 * n * h * w + (n * h * w if e else 0)),
    'davis_counts': lambda n, h, w, o, s, e: davis_need(n, h, w, o),
}
# stage -> the regions that start out as 0, in layout order
CLEARED = {
    'label_components': [], 'block_motion': [], 'crf_labels': [], 'distance_sq': [],
    'filter_components': ['area', 'best', 'removed', 'cand', 'pres'],
    'fill_holes': ['area', 'rec', 'cnt', 'hist', 'filled', 'pres'],
    'superpixels': ['sums'],
    'snap_labels': ['sums', 'votes', 'changed'],
    'adapt_targets': ['count_e', 'n_pos'],
    'davis_counts': ['counts'],
}
# stage -> (frames_per_call(h, w, n_obj, step, erode) of the Python module that chunks for it, whether that formula is exact,
# the most frames the entry point takes)
CHUNK = {
    'label_components': (lambda h, w, o, s, e: components.frames_per_call(h, w), False, 65535),
    'filter_components': (lambda h, w, o, s, e: components.frames_per_call(h, w), True, 65535),
    'fill_holes': (lambda h, w, o, s, e: holes.frames_per_call(h, w), True, 65535),
    'superpixels': (lambda h, w, o, s, e: snap.frames_per_call(0, h, w, s), False, 65535),
    'snap_labels': (lambda h, w, o, s, e: snap.frames_per_call(o, h, w, s), False, 65535),
    'block_motion': (lambda h, w, o, s, e: motion.frames_per_call(h, w), True, 65534),
    'crf_labels': (lambda h, w, o, s, e: crf.frames_per_call(o, h, w), True, 65535),
    'distance_sq': (lambda h, w, o, s, e: adapt.frames_per_call(h, w), False, 65535),
    'adapt_targets': (lambda h, w, o, s, e: adapt.frames_per_call(h, w, e), True, 65535),
}
SMALL = [(1, 1, 1), (1, 7, 9), (3, 37, 53), (5, 97, 161)]
DAVIS = [(480, 854), (1080, 1920), (4096, 4095)]


def cases():
    """Every (stage, n, h, w, n_obj, step, erode) of the test, the ones at and just past `frames_per_call` included."""
    out = []
    for stage in NEED:
        for e in ((0, 1) if stage == 'adapt_targets' else (0,)):
            out += [(stage, n, h, w, 3, 16, e) for n, h, w in SMALL]
            out += [(stage, 2, 33, 65, o, s, e) for o in (1, 3, 255) for s in (4, 16, 64)]
            for h, w in DAVIS:
                if stage == 'davis_counts':
                    out += [(stage, n, h, w, o, 16, e) for n in (1, 8, 100) for o in (1, 3)]
                    continue
                fpc, _, most = CHUNK[stage]
                for o, s in ((1, 16), (3, 4), (3, 16)):
                    n = fpc(h, w, o, s, e)
                    out += [(stage, m, h, w, o, s, e) for m in (1, n, n + 1) if m <= most]
    return sorted(set(out))


@pytest.fixture(scope='module')
def layouts(tmp_path_factory):
    """{case: ([(name, offset, bytes, element bytes)], need, clear offset, clear bytes)} as the sanitised program printed them."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('scratch_layout') / 'scratch_layout_main')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tests', 'host', 'scratch_layout_main.cpp'), '-o', exe], check=True)
    want = cases()
    p = subprocess.run([exe] + [','.join(map(str, c)) for c in want], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    got = {}
    for line in p.stdout.splitlines():
        key, kind, *rest = line.split()
        c = key.split(',')
        c = (c[0],) + tuple(int(v) for v in c[1:])
        entry = got.setdefault(c, [[], None, None, None])
        if kind == 'region':
            entry[0].append((rest[0], int(rest[1]), int(rest[2]), int(rest[3])))
        else:
            entry[1:] = [int(rest[0]), int(rest[2]), int(rest[3])]
    assert sorted(got) == want
    return got


def test_regions_are_in_bounds_disjoint_and_aligned(layouts):
    for c, (regions, need, _, _) in layouts.items():
        assert regions and need % 4 == 0, c
        end = 0
        for name, at, size, elem in regions:                          # in layout order: disjoint means no region starts early
            assert at >= end and at % elem == 0 and size % elem == 0 and at + size <= need, (c, name)
            end = at + size
        assert len({r[0] for r in regions}) == len(regions), c


def test_the_cleared_range_is_the_one_the_entry_points_always_cleared(layouts):
    for c, (regions, need, clear_at, clear_bytes) in layouts.items():
        by_name = {r[0]: r for r in regions}
        names = CLEARED[c[0]]
        assert set(names) <= set(by_name), c
        if not names:
            assert clear_bytes == 0, c
            continue
        assert clear_at == by_name[names[0]][1], c                    # from the first cleared region ...
        assert clear_at + clear_bytes == by_name[names[-1]][1] + by_name[names[-1]][2] <= need, c       # ... to the end of the last
        for name, at, size, _ in regions:
            inside = clear_at <= at and at + size <= clear_at + clear_bytes
            outside = at + size <= clear_at or at >= clear_at + clear_bytes
            assert (inside if name in names else outside or size == 0), (c, name)


def test_need_is_what_the_entry_points_computed_before(layouts):
    for c, (_, need, _, _) in layouts.items():
        assert need == NEED[c[0]](*c[1:]), c


def test_the_python_modules_chunk_under_the_cap(layouts):
    """`need(frames_per_call) <= 512 MB` whenever one frame fits; where the Python formula is exact, one frame more does not."""
    seen = 0
    for c, (_, need, _, _) in layouts.items():
        stage, n, h, w, o, s, e = c
        if stage not in CHUNK or (h, w) not in DAVIS:
            continue
        fpc, exact, most = CHUNK[stage]
        step = fpc(h, w, o, s, e)
        one = layouts[(stage, 1, h, w, o, s, e)][1]
        if n == step and one <= CAP:
            assert need <= CAP, c
            seen += 1
        if n == step + 1 and exact and step < most:
            assert need > CAP, c
            seen += 1
    assert seen >= 2 * len(CHUNK)
