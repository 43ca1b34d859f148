"""Reader and writer of the object checkpoint format, written from DESIGN.md 3.7 alone (struct + numpy, no library call): what the tests hold
mon_object_save / mon_object_load / mon_checkpoint_read_info against.  Everything is little-endian."""
import struct
import zlib

import numpy as np

MAGIC = b"MONCKPT\0"
VERSION = 1
HEADER_BYTES, OBJECT_OFF, STATE_OFF, TABLE_OFF, ENTRY_BYTES = 64, 64, 320, 448, 32
F32, U32, F16, BBOX = 1, 2, 3, 4
ELEM_BYTES = {F32: 4, U32: 4, F16: 2, BBOX: 20}
DTYPES = {F32: "<f4", U32: "<u4", F16: "<u2", BBOX: "<u4"}

# the object block's config part: (name, struct code) in file order; a zero word sits between occupancy_skip and the 64-bit sample_seed
CONFIG_FIELDS = [("n_levels", "i"), ("n_features", "i"), ("log2_hashmap_size", "i"), ("base_resolution", "i"), ("per_level_scale", "f"), ("n_neurons", "i"),
                 ("n_hidden_layers", "i"), ("rays_per_batch", "i"), ("n_samples", "i"), ("loss_scale", "f"), ("learning_rate", "f"), ("beta1", "f"),
                 ("beta2", "f"), ("epsilon", "f"), ("l2_reg", "f"), ("ema_decay", "f"), ("decay_start", "i"), ("decay_interval", "i"), ("decay_base", "f"),
                 ("param_seed", "I"), ("rng_flags", "I"), ("use_depth", "i"), ("occupancy_skip", "i")]
# the state block's 32-bit words, in file order (floats as their bits); the rest of the block's 32 words is zero
STATE_WORDS = ["step", "iter", "skipped", "lr", "n_valid", "loss_sum", "n_valid_pre", "n_scatter_now", "n_scatter_last", "n_scatter_total", "ema_deb_old",
               "ema_deb_new", "ema_deb_even_old", "ema_deb_even_new", "occ_refreshed_iter", "occ_next_refresh", "occ_raw_threshold", "ema_pending"]
STATE_FLOATS = {"lr", "loss_sum", "ema_deb_old", "ema_deb_new", "ema_deb_even_old", "ema_deb_even_new", "occ_raw_threshold"}


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def from_bits(u):
    return struct.unpack("<f", struct.pack("<I", u))[0]


def section_order(obj):
    """Tags (type, count) a file of this object block holds, in file order."""
    n = obj["n_params"]
    out = [("master", F32, n), ("m1", F32, n), ("m2", F32, n), ("steps", U32, n), ("ema", F16, n)]
    if obj["lazy_ema"]:
        out.append(("ema_step", U32, n // 8))
    if obj["has_occupancy"]:
        out += [("occ", U32, 8192), ("occ_raw", U32, 8192)]
    out.append(("boxes", BBOX, obj["n_boxes"]))
    return out


def write(path, cfg, obj, state, sections):
    """cfg: dict of every mon_config field; obj: class_id, Tow (16), aabb_min, aabb_max, n_params, n_mlp_params, n_grid_params, backend, step_bits,
    lazy_ema, has_occupancy, n_boxes; state: dict of STATE_WORDS (floats as floats; missing = 0); sections: tag -> numpy array."""
    order = section_order(obj)
    head_len = TABLE_OFF + ENTRY_BYTES * len(order)
    blobs, table, off = [], [], head_len
    for tag, typ, count in order:
        a = np.ascontiguousarray(sections[tag]).astype(DTYPES[typ], copy=False).reshape(-1)
        raw = a.tobytes()
        assert len(raw) == count * ELEM_BYTES[typ], (tag, len(raw), count)
        off = (off + 63) & ~63
        table.append((tag, typ, zlib.crc32(raw) & 0xffffffff, count, off)); blobs.append((off, raw)); off += len(raw)
    file_bytes = off
    h = bytearray(head_len)
    h[0:8] = MAGIC
    struct.pack_into("<IIQI", h, 8, VERSION, len(order), file_bytes, TABLE_OFF)
    o = OBJECT_OFF
    for name, code in CONFIG_FIELDS:
        struct.pack_into("<" + code, h, o, cfg[name]); o += 4
    struct.pack_into("<IQ", h, o, 0, cfg["sample_seed"]); o += 12
    struct.pack_into("<i", h, o, obj["class_id"]); o += 4
    struct.pack_into("<16f", h, o, *[float(v) for v in obj["Tow"]]); o += 64
    struct.pack_into("<3f", h, o, *[float(v) for v in obj["aabb_min"]]); o += 12
    struct.pack_into("<3f", h, o, *[float(v) for v in obj["aabb_max"]]); o += 12
    struct.pack_into("<IIIiIIII", h, o, obj["n_params"], obj["n_mlp_params"], obj["n_grid_params"], obj["backend"], obj["step_bits"], obj["lazy_ema"],
                     obj["has_occupancy"], obj["n_boxes"])
    for k, name in enumerate(STATE_WORDS):
        v = state.get(name, 0)
        struct.pack_into("<I", h, STATE_OFF + 4 * k, bits(v) if name in STATE_FLOATS else int(v))
    for k, (tag, typ, crc, count, soff) in enumerate(table):
        e = TABLE_OFF + ENTRY_BYTES * k
        h[e:e + len(tag)] = tag.encode()
        struct.pack_into("<IIQQ", h, e + 8, typ, crc, count, soff)
    struct.pack_into("<I", h, 28, zlib.crc32(bytes(h)) & 0xffffffff)          # over [0, table end) with this field still zero
    with open(path, "wb") as f:
        f.write(bytes(h))
        for soff, raw in blobs:
            f.write(b"\0" * (soff - f.tell())); f.write(raw)
    return dict(file_bytes=file_bytes, head_len=head_len, table=table)


def read(path, verify=True):
    """-> dict(version, file_bytes, cfg, obj, state (floats decoded, plus state_bits), table, sections: tag -> numpy array)."""
    raw = open(path, "rb").read()
    assert raw[:8] == MAGIC, "bad magic"
    version, n_sec, file_bytes, table_off = struct.unpack_from("<IIQI", raw, 8)
    assert version == VERSION and table_off == TABLE_OFF and file_bytes == len(raw), (version, table_off, file_bytes, len(raw))
    head_len = TABLE_OFF + ENTRY_BYTES * n_sec
    stored = struct.unpack_from("<I", raw, 28)[0]
    h = bytearray(raw[:head_len]); struct.pack_into("<I", h, 28, 0)
    assert zlib.crc32(bytes(h)) & 0xffffffff == stored, "header CRC"
    cfg, o = {}, OBJECT_OFF
    for name, code in CONFIG_FIELDS:
        cfg[name] = struct.unpack_from("<" + code, raw, o)[0]; o += 4
    cfg["sample_seed"] = struct.unpack_from("<Q", raw, o + 4)[0]; o += 12
    obj = dict(class_id=struct.unpack_from("<i", raw, o)[0]); o += 4
    obj["Tow"] = np.array(struct.unpack_from("<16f", raw, o), np.float32); o += 64
    obj["aabb_min"] = np.array(struct.unpack_from("<3f", raw, o), np.float32); o += 12
    obj["aabb_max"] = np.array(struct.unpack_from("<3f", raw, o), np.float32); o += 12
    for name, v in zip(("n_params", "n_mlp_params", "n_grid_params", "backend", "step_bits", "lazy_ema", "has_occupancy", "n_boxes"),
                       struct.unpack_from("<IIIiIIII", raw, o)):
        obj[name] = v
    words = struct.unpack_from("<%dI" % len(STATE_WORDS), raw, STATE_OFF)
    state_bits = dict(zip(STATE_WORDS, words))
    state = {k: (from_bits(v) if k in STATE_FLOATS else v) for k, v in state_bits.items()}
    table, sections = [], {}
    for k in range(n_sec):
        e = TABLE_OFF + ENTRY_BYTES * k
        tag = raw[e:e + 8].rstrip(b"\0").decode()
        typ, crc, count, soff = struct.unpack_from("<IIQQ", raw, e + 8)
        assert soff % 64 == 0 and soff + count * ELEM_BYTES[typ] <= len(raw), (tag, soff, count)
        blob = raw[soff:soff + count * ELEM_BYTES[typ]]
        if verify:
            assert zlib.crc32(blob) & 0xffffffff == crc, "CRC of section " + tag
        a = np.frombuffer(blob, DTYPES[typ]).copy()
        sections[tag] = a.reshape(-1, 5) if typ == BBOX else a
        table.append((tag, typ, crc, count, soff))
    assert [(t[0], t[1], t[3]) for t in table] == section_order(obj), "section list"
    return dict(version=version, file_bytes=file_bytes, cfg=cfg, obj=obj, state=state, state_bits=state_bits, table=table, sections=sections)
