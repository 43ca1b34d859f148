"""Checkpoint file format on the host: a file produced by the Python writer of tests/checkpoint_format.py -- written from the document, not
from the library -- is read by mon_checkpoint_read_info with every field equal, and every kind of damage is a clean MON_ERR_IO with a message."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import checkpoint_format as cf
from conftest import C1

MON_ERR_IO = 4


def c1_config(pkg):
    return pkg.default_config(**dict(C1, decay_start=20, decay_interval=10))


def config_dict(pkg, cfg):
    return {f: getattr(cfg, f) for f, _ in pkg.MonConfig._fields_}


def param_counts(pkg, orc, cfg):
    """(n_mlp, n_grid) of a config: the MLP's padded matrices (W x Epad, (NH - 1) W x W, 16 x W) and tcnn's level table times two features."""
    ocfg = orc.default_config(**{f: getattr(cfg, f) for f in ("n_levels", "n_features", "log2_hashmap_size", "base_resolution", "per_level_scale")})
    off = np.zeros(33, np.uint32); sc = np.zeros(32, np.float32); res = np.zeros(32, np.uint32)
    orc.lib().orc_level_table(C.byref(ocfg), off.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p))
    W, NH, epad = cfg.n_neurons, cfg.n_hidden_layers, (16 if 2 * cfg.n_levels <= 16 else 32)
    return W * epad + (NH - 1) * W * W + 16 * W, 2 * int(off[cfg.n_levels])


@pytest.fixture(scope="module")
def good(pkg, orc, tmp_path_factory):
    """C1's config, zero state, 3 boxes, written by the Python writer."""
    cfg = c1_config(pkg); n_mlp, n_grid = param_counts(pkg, orc, cfg); n = n_mlp + n_grid
    obj = dict(class_id=7, Tow=np.arange(16, dtype=np.float32) * 0.25 - 1.0, aabb_min=[-0.5, -0.25, -0.125], aabb_max=[0.5, 0.25, 0.125], n_params=n,
               n_mlp_params=n_mlp, n_grid_params=n_grid, backend=1, step_bits=16, lazy_ema=0, has_occupancy=0, n_boxes=3)
    state = dict(lr=cfg.learning_rate, ema_deb_new=1.0 / (1.0 - cfg.ema_decay))
    sections = dict(master=np.zeros(n, np.float32), m1=np.zeros(n, np.float32), m2=np.zeros(n, np.float32), steps=np.zeros(n, np.uint32),
                    ema=np.zeros(n, np.uint16), boxes=np.array([[0, 1, 2, 30, 40], [3, 0, 0, 120, 160], [11, 5, 6, 7, 8]], np.uint32))
    path = str(tmp_path_factory.mktemp("ckpt") / "c1.monckpt")
    lay = cf.write(path, config_dict(pkg, cfg), obj, state, sections)
    return dict(path=path, cfg=cfg, obj=obj, lay=lay, raw=open(path, "rb").read())


def test_python_written_file_is_read_with_every_field_equal(pkg, good):
    i = pkg.checkpoint_info(good["path"], verify=True)
    cfg, obj = good["cfg"], good["obj"]
    for f, _ in pkg.MonConfig._fields_:
        assert getattr(i.cfg, f) == getattr(cfg, f), f
    assert i.version == 1 and i.class_id == obj["class_id"] and i.file_bytes == len(good["raw"]) == good["lay"]["file_bytes"]
    assert np.array_equal(np.array(i.Tow[:], np.float32), obj["Tow"])
    assert list(i.aabb_min) == obj["aabb_min"] and list(i.aabb_max) == obj["aabb_max"]
    assert (i.n_params, i.n_mlp_params, i.n_grid_params) == (obj["n_params"], obj["n_mlp_params"], obj["n_grid_params"])
    assert (i.train_step, i.iter, i.n_boxes, i.backend, i.has_occupancy, i.lazy_ema) == (0, 0, 3, 1, 0, 0)
    # and the Python reader agrees with its own writer
    back = cf.read(good["path"])
    assert back["obj"]["n_boxes"] == 3 and np.array_equal(back["sections"]["boxes"][2], [11, 5, 6, 7, 8]) and back["cfg"]["decay_start"] == 20


def refresh_head_crc(b, n_sections):
    """The header CRC recomputed after a deliberate edit of a field it covers (the damage under test is then the field, not the CRC)."""
    end = cf.TABLE_OFF + cf.ENTRY_BYTES * n_sections
    struct.pack_into("<I", b, 28, 0); struct.pack_into("<I", b, 28, zlib.crc32(bytes(b[:end])) & 0xffffffff)


def damaged_files(good):
    """(name, bytes, verify needed) of every damaged variant of the good file."""
    raw = good["raw"]; table = good["lay"]["table"]; ns = len(table); out = []
    out.append(("cut mid-header", raw[:40], False)); out.append(("cut in the object block", raw[:200], False)); out.append(("empty", b"", False))
    out.append(("cut in the section table", raw[:cf.TABLE_OFF + 40], False))
    for tag, typ, crc, count, off in table:
        out.append(("cut at the start of " + tag, raw[:off], False))
        out.append(("cut at the end of " + tag, raw[:off + count * cf.ELEM_BYTES[typ] - 1], False))
    b = bytearray(raw); b[0] ^= 0x20; out.append(("bad magic", bytes(b), False))
    b = bytearray(raw); struct.pack_into("<I", b, 8, 2); refresh_head_crc(b, ns); out.append(("version 2", bytes(b), False))
    b = bytearray(raw); b[cf.OBJECT_OFF + 41] ^= 0x04; out.append(("flipped byte in the header", bytes(b), False))
    b = bytearray(raw); b[cf.STATE_OFF + 2] ^= 0x80; out.append(("flipped byte in the state block", bytes(b), False))
    for tag, typ, crc, count, off in table:
        b = bytearray(raw); b[off + (count * cf.ELEM_BYTES[typ]) // 2] ^= 0x01; out.append(("flipped byte in " + tag, bytes(b), True))
    b = bytearray(raw); struct.pack_into("<Q", b, cf.TABLE_OFF + cf.ENTRY_BYTES * 1 + 24, (len(raw) + 63) & ~63); refresh_head_crc(b, ns)
    out.append(("section offset past EOF", bytes(b), False))
    b = bytearray(raw); struct.pack_into("<I", b, cf.OBJECT_OFF + 196, good["obj"]["n_params"] + 8); refresh_head_crc(b, ns)
    out.append(("n_params off by 8", bytes(b), False))
    b = bytearray(raw); struct.pack_into("<i", b, cf.OBJECT_OFF + 4, 3); refresh_head_crc(b, ns); out.append(("n_features = 3", bytes(b), False))
    return out


def test_damaged_files_are_io_errors_not_crashes(pkg, good, tmp_path):
    f = tmp_path / "bad.monckpt"; n = 0
    for name, data, needs_verify in damaged_files(good):
        f.write_bytes(data)
        with pytest.raises(pkg.MonError) as e:
            pkg.checkpoint_info(str(f), verify=True)
        assert e.value.code == MON_ERR_IO and len(str(e.value)) > 25, (name, str(e.value))
        if needs_verify:                      # a flipped section byte is only seen by the section CRCs
            assert pkg.checkpoint_info(str(f), verify=False).n_boxes == 3, name
        else:
            with pytest.raises(pkg.MonError) as e2:
                pkg.checkpoint_info(str(f), verify=False)
            assert e2.value.code == MON_ERR_IO, name
        n += 1
    assert n >= 24
    with pytest.raises(pkg.MonError) as e:
        pkg.checkpoint_info(str(tmp_path / "missing.monckpt"))
    assert e.value.code == MON_ERR_IO
    rc = pkg.lib().mon_checkpoint_read_info(None, 1, None)
    assert rc == 1                                                            # MON_ERR_ARG


def test_random_damage_never_crashes(pkg, good, tmp_path):
    """test_config_reader_survives_damaged_files's style: truncations and byte flips anywhere give a clean error or, for flips the CRCs cannot see
    (none: every byte is covered or padding), the unchanged info."""
    raw = good["raw"]; rs = np.random.RandomState(0); f = tmp_path / "m.monckpt"
    pad = np.ones(len(raw), bool)
    pad[:good["lay"]["head_len"]] = False
    for tag, typ, crc, count, off in good["lay"]["table"]:
        pad[off:off + count * cf.ELEM_BYTES[typ]] = False
    for cut in list(range(0, 600, 7)) + [int(v) for v in rs.randint(600, len(raw), 40)]:
        f.write_bytes(raw[:cut])
        with pytest.raises(pkg.MonError) as e:
            pkg.checkpoint_info(str(f))
        assert e.value.code == MON_ERR_IO
    for _ in range(150):
        b = bytearray(raw); pos = int(rs.randint(0, 600)) if rs.rand() < 0.7 else int(rs.randint(0, len(raw)))
        b[pos] ^= 1 << int(rs.randint(0, 8)); f.write_bytes(bytes(b))
        if pad[pos]:
            assert pkg.checkpoint_info(str(f)).n_boxes == 3
        else:
            with pytest.raises(pkg.MonError) as e:
                pkg.checkpoint_info(str(f))
            assert e.value.code == MON_ERR_IO, pos
