"""The operator decision of prcg_set_csr as a host-only function (csrc/prcg_plan.cpp: plan_operator), through the test hook
prcg_plan_operator: which kernel family an operator gets, with which encodings, and -- by four FNV-1a hashes -- every byte
of the index streams, value-index streams, dictionaries and tile tables an upload would copy.  No GPU, no handle.

The families / encodings asserted here are the ones the GPU tests assert through schedule() (tests/test_xp_deferred.py:
OPERATORS; tests/test_gpu_configs.py: test_window_kernels_selected_for_bands_and_stencils_only).

REFERENCE.  The EXPECTED rows below were recorded from the commit BEFORE plan_operator existed (9d2fd29): that commit's
prcg_set_csr, unchanged, was compiled into a scratch library in which the device buffers were host allocations and
hipMemcpy a memcpy that remembers how many bytes each buffer received; the hook hashed exactly those bytes, buffer by
buffer in the order documented in include/prcg_test.h, and reported the handle's flags.  They are the reference for "byte
for byte as before" and are never regenerated from the code under test."""
import pytest

from new_cg_variants_amd import device, partition, problems as P


def _s1_block(rank):
    return partition.split_serial(P.WORKLOADS['s1_small']['make'](), 2)[1][rank][0]


SOURCES = {
    'band': lambda: P.WORKLOADS['s3_small']['make'](),        # ex2b band, 15 diagonals, n = 20,000
    'band_long': lambda: P.banded_ex2b(280_000, 7),           # more than 4096 interior window tiles: the image-period search runs
    'lap2d': lambda: P.laplace_2d(130, 77),
    'lap3d': lambda: P.laplace_3d(24, 20, 18),
    'fem': lambda: P.fem_like_3d(12, 3),
    'irregular': lambda: P.irregular_standin(6000),
    's1_block0': lambda: _s1_block(0),                        # s1_small as two row blocks: ghost columns, boundary tiles
    's1_block1': lambda: _s1_block(1),
}

# (source, knobs) -> the 18 values of device.PLAN_OPERATOR_FIELDS, recorded from the parent commit (see above)
EXPECTED = {
    ('band_long', ()):
        (1, 0, 64, 0, 0, 1, 1, 1, 1, 2, 4375, 0, 0, 436750,
         0xf99df496e53a2df7, 0x66c4c1fb89a45813, 0x9cf95bda8de1e627, 0xcc1c5bef9084394c),
    ('lap3d', (('PRCG_WIN_SWEEP', '2'),)):
        (1, 5, 64, 1, 0, 1, 1, 0, 0, 1, 135, 0, 0, 15640,
         0x76c4f5b0bf5a4bf7, 0xb9b23f3a46fd0825, 0xeb16e62ed5b43245, 0x99c49ce39457bc56),
    ('lap2d', (('PRCG_SWEEP_WAVES', '64'), ('PRCG_WIN_SWEEP', '2'))):
        (1, 5, 64, 1, 0, 1, 1, 0, 0, 1, 157, 0, 0, 20512,
         0xf0350648ba18dedc, 0xb9b23f3a46fd0825, 0xddb0fe5fe6336e27, 0xec48efe74fef0e13),
    ('band', ()):
        (1, 0, 64, 0, 0, 1, 1, 1, 1, 2, 313, 0, 0, 45774,
         0xe53f678cb4cdab54, 0xac659d5367888efd, 0x649b1f6192d6aefa, 0xee44e01aeda0cf0f),
    ('band', (('PRCG_VALDICT', '0'),)):
        (1, 0, 64, 0, 0, 0, 0, 1, 1, 2, 313, 0, 0, 2432318,
         0xe53f678cb4cdab54, 0xcbf29ce484222325, 0xcbf29ce484222325, 0xdcf372b62f9fcd21),
    ('band', (('PRCG_WIN', '0'),)):
        (0, -1, 0, 0, 0, 1, 0, 1, 4, 2, 606, 0, 0, 699284,
         0x5aab5296502cd2db, 0x9b4d45a981c8e50c, 0x86b49264947acc24, 0x242538c61dd6f96a),
    ('band', (('PRCG_WIN', '0'), ('PRCG_COL8', '0'))):
        (0, -1, 0, 0, 0, 1, 0, 2, 4, 2, 606, 0, 0, 999228,
         0x1819d77c65b35837, 0x9b4d45a981c8e50c, 0x86b49264947acc24, 0x242538c61dd6f96a),
    ('band', (('PRCG_WIN', '0'), ('PRCG_VALDICT', '0'), ('PRCG_COL16', '0'))):
        (0, -1, 0, 0, 0, 0, 0, 4, 4, 2, 606, 0, 0, 3689028,
         0x654cfc17ed01b555, 0xcbf29ce484222325, 0xcbf29ce484222325, 0x242538c61dd6f96a),
    ('band', (('PRCG_WIN_SHARE', '0'),)):
        (1, 0, 64, 0, 0, 1, 1, 1, 1, 2, 313, 0, 0, 678394,
         0x4240c014b5095bd4, 0x483fe10ec56882bd, 0x649b1f6192d6aefa, 0x7c7c7663cc978a95),
    ('lap2d', ()):
        (1, 5, 64, 1, 0, 1, 1, 0, 0, 1, 157, 0, 0, 20512,
         0xf0350648ba18dedc, 0xb9b23f3a46fd0825, 0xddb0fe5fe6336e27, 0xec48efe74fef0e13),
    ('lap2d', (('PRCG_WIN_SWEEP', '2'),)):
        (1, 5, 64, 1, 0, 1, 1, 0, 0, 1, 157, 0, 0, 20512,
         0xf0350648ba18dedc, 0xb9b23f3a46fd0825, 0xddb0fe5fe6336e27, 0xec48efe74fef0e13),
    ('lap2d', (('PRCG_WIN', '0'),)):
        (0, -1, 0, 0, 0, 1, 0, 2, 4, 1, 198, 0, 0, 195288,
         0x21da6a4266abdf9a, 0x8a27a3f9c0ca12d8, 0x1255cc0cd862e317, 0xcf513a6c0de42fa5),
    ('lap3d', ()):
        (1, 5, 64, 1, 0, 1, 1, 0, 0, 1, 135, 0, 0, 15640,
         0x76c4f5b0bf5a4bf7, 0xb9b23f3a46fd0825, 0xeb16e62ed5b43245, 0x99c49ce39457bc56),
    ('lap3d', (('PRCG_WIN_PAT', '0'),)):
        (1, 2, 128, 0, 0, 1, 1, 2, 2, 1, 68, 0, 0, 50446,
         0x323bb42aca45daf5, 0xbecab37f0bc01e30, 0xc2d4a261537ed4a5, 0x9e7cd7b6917eaba1),
    ('lap3d', (('PRCG_VALDICT', '0'), ('PRCG_WIN_PAT', '0'))):
        (1, 2, 128, 0, 0, 0, 0, 2, 2, 1, 68, 0, 0, 500526,
         0x323bb42aca45daf5, 0xcbf29ce484222325, 0xcbf29ce484222325, 0x56e305cab27a635),
    ('lap3d', (('PRCG_WIN_ROWS', '128'),)):
        (1, 2, 128, 0, 0, 1, 1, 2, 2, 1, 68, 0, 0, 50446,
         0x323bb42aca45daf5, 0xbecab37f0bc01e30, 0xc2d4a261537ed4a5, 0x9e7cd7b6917eaba1),
    ('fem', ()):
        (2, -1, 0, 0, 0, 0, 0, 2, 2, 4, 81, 0, 0, 3503476,
         0x6a4dd6d339508507, 0xcbf29ce484222325, 0x7fd1fff4c771748, 0xad68b90104bb2c91),
    ('fem', (('PRCG_SELL', '0'),)):
        (0, -1, 0, 0, 0, 0, 0, 2, 4, 4, 364, 0, 0, 3563924,
         0x2d678cd132a920a1, 0xcbf29ce484222325, 0xcbf29ce484222325, 0xbb66fd2c03b75377),
    ('fem', (('PRCG_SELL_WINDOW', '0'),)):
        (2, -1, 0, 0, 0, 0, 0, 2, 2, 4, 81, 0, 0, 3290404,
         0x350595cbb36ae229, 0xcbf29ce484222325, 0xc82ec5f306ad5a0, 0xce21481689150684),
    ('irregular', ()):
        (0, -1, 0, 0, 0, 0, 0, 2, 4, 1, 182, 0, 0, 595156,
         0x989357f6fc850d23, 0xcbf29ce484222325, 0xcbf29ce484222325, 0xe948213008b2a827),
    ('irregular', (('PRCG_TILE_STEPS', '1'),)):
        (0, -1, 0, 0, 0, 0, 0, 2, 4, 1, 182, 0, 0, 595156,
         0x989357f6fc850d23, 0xcbf29ce484222325, 0xcbf29ce484222325, 0xe948213008b2a827),
    ('s1_block0', ()):
        (1, 5, 64, 1, 0, 1, 1, 0, 0, 1, 23, 1, 0, 2832,
         0x5143d4a7c92b23ca, 0xb9b23f3a46fd0825, 0xc439f2cc34822615, 0x81d358c408aac915),
    ('s1_block1', ()):
        (1, 5, 64, 1, 0, 1, 1, 0, 0, 1, 23, 1, 0, 2904,
         0x8a34ac7d96bc8d25, 0xb9b23f3a46fd0825, 0xea21d8b1d99579c3, 0xe0fd827c6c695d67),
    ('s1_block0', (('PRCG_WIN', '0'),)):
        (0, -1, 0, 0, 0, 1, 1, 1, 1, 1, 29, 2, 0, 22276,
         0x28694bd14be843a9, 0x8f88431e190a1542, 0x7b0e4f142983c114, 0xe7caa8fc6c0f92fc),
    ('s1_block1', (('PRCG_WIN', '0'),)):
        (0, -1, 0, 0, 0, 1, 1, 1, 2, 1, 29, 2, 0, 22276,
         0xaff7f00853794c42, 0xf7091b49e67f1245, 0x295714669b87db4, 0x7521cfd0131d29e8),
    ('s1_block1', (('PRCG_WIN_PAT', '0'),)):
        (1, 2, 128, 0, 0, 1, 1, 2, 2, 1, 12, 1, 0, 11296,
         0x9fe3c55d2f13abd5, 0x610681481d31d9dd, 0xe406ebb469aa4868, 0xf3c837a8311e5d14),
}

_cache = {}


def operator(source):
    if source not in _cache:
        _cache[source] = SOURCES[source]()
    return _cache[source]


def plan(source, knobs):
    return device.plan_operator(operator(source), dict(knobs))


@pytest.mark.parametrize('source,knobs', sorted(EXPECTED))
def test_plan_equals_parent_byte_for_byte(source, knobs):
    got = plan(source, knobs)
    want = dict(zip(device.PLAN_OPERATOR_FIELDS, EXPECTED[(source, knobs)]))
    assert got == want, {f: (got[f], want[f]) for f in got if got[f] != want[f]}


# tests/test_xp_deferred.py: OPERATORS -- operator, knobs, bytes per window index or None, value dictionary or None, pattern tiles
@pytest.mark.parametrize('source,knobs,col_bytes,value_dict,pattern', [
    ('band', {}, 1, True, False),
    ('band', {'PRCG_VALDICT': '0'}, 1, False, False),
    ('lap3d', {'PRCG_WIN_PAT': '0'}, 2, None, False),
    ('lap3d', {'PRCG_WIN_PAT': '0', 'PRCG_VALDICT': '0'}, 2, False, False),
    ('lap2d', {}, None, True, True),
    ('lap3d', {}, None, True, True),
])
def test_window_operators_as_the_gpu_tests_see_them(source, knobs, col_bytes, value_dict, pattern):
    got = device.plan_operator(operator(source), knobs)
    assert got['family'] == 1 and bool(got['pattern']) == pattern, got
    assert got['rows_per_tile'] in (64, 128) and got['tiles_interior'] > 0 and got['tiles_boundary'] == 0, got
    if col_bytes is not None:
        assert got['col_bytes'] == col_bytes, got
    if value_dict is not None:
        assert bool(got['value_dict']) == value_dict, got
    if pattern:
        assert got['win_geom'] == 5 and got['rows_per_tile'] == 64 and got['col_bytes'] == 0, got


def test_sliced_rows_classic_tiles_and_boundary_tiles():
    fem = device.plan_operator(operator('fem'))
    assert fem['family'] == 2 and fem['col_bytes'] == 2 and fem['tiles_interior'] > 0, fem      # test_gpu_configs: 'fem'
    off = device.plan_operator(operator('band'), {'PRCG_WIN': '0'})
    assert off['family'] == 0 and off['win_geom'] == -1 and off['col_bytes'] == 1 and off['value_dict'], off
    irr = device.plan_operator(operator('irregular'))
    assert irr['family'] != 1, irr                   # mean row length 76: no window operator
    for rank in (0, 1):
        blk = operator(f's1_block{rank}')
        assert blk.shape[1] > blk.shape[0]
        for knobs in ({}, {'PRCG_WIN': '0'}):
            got = device.plan_operator(blk, knobs)
            assert got['tiles_boundary'] > 0 and got['tiles_interior'] > 0, (rank, knobs, got)
            assert got['family'] == (0 if knobs else 1), (rank, knobs, got)


def test_unknown_option_is_refused():
    with pytest.raises(RuntimeError):
        device.plan_operator(operator('lap2d'), {'PRCG_NO_SUCH_SWITCH': '1'})
