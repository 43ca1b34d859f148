"""Store policies of the training hand-over buffers (ro-map_amd/csrc/store_policy.h) and the reordered entry of k_grid_scatter.

A store's cache policy decides when its bytes leave the L2, never what they are, so every check here is bit-for-bit:
  * CPU: the header compiles for gfx950 with every policy at every width;
  * GPU: a batch without a valid ray leaves every parameter and optimizer array untouched and is counted as skipped (k_grid_scatter now clears its
    tile before it knows whether the batch is skipped);
  * GPU: the shipped library and a variant with every policy forced to plain stores train the bench object to the same parameters."""
import json
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ro-map_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
POLICIES = ["MON_SP_PLAIN", "MON_SP_NT", "MON_SP_WT", "MON_SP_WT_NT"]

PROBE = """
#include "store_policy.h"
typedef _Float16 h1; typedef _Float16 h2 __attribute__((ext_vector_type(2))); typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8))); typedef float f4 __attribute__((ext_vector_type(4)));
template <int P> __device__ void all_widths(h1* a, h2* b, float* c, h4* d, h8* e, f4* f, unsigned i) {
    mon::policy_store<P>(a[i + 1], a + i); mon::policy_store<P>(b[i + 1], b + i); mon::policy_store<P>(c[i + 1], c + i);
    mon::policy_store<P>(d[i + 1], d + i); mon::policy_store<P>(e[i + 1], e + i); mon::policy_store<P>(f[i + 1], f + i);
}
__global__ void k_probe(h1* a, h2* b, float* c, h4* d, h8* e, f4* f) {
    const unsigned i = 2u * (blockIdx.x * blockDim.x + threadIdx.x);
    all_widths<MON_SP_PLAIN>(a, b, c, d, e, f, i); all_widths<MON_SP_NT>(a + 4096, b + 4096, c + 4096, d + 4096, e + 4096, f + 4096, i);
    all_widths<MON_SP_WT>(a + 8192, b + 8192, c + 8192, d + 8192, e + 8192, f + 8192, i);
    all_widths<MON_SP_WT_NT>(a + 12288, b + 12288, c + 12288, d + 12288, e + 12288, f + 12288, i);
}
"""


def test_store_policy_header_compiles_every_policy_and_width(tmp_path):
    """store_policy.h, --offload-arch=gfx950, policies plain / nt / wt / wt_nt at 2, 4, 8 and 16 bytes per lane: compiles, and the device code carries
    as many stores as were asked for (no policy silently falls back to another width or is dropped)."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    src = tmp_path / "probe.hip"; src.write_text(PROBE)
    asm = tmp_path / "probe.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-I", CSRC, "--cuda-device-only", "-S", str(src), "-o", str(asm)])
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-I", CSRC, "-c", str(src), "-o", str(tmp_path / "probe.o")])
    lines = [ln.split(";")[0] for ln in asm.read_text().splitlines() if "_store_" in ln.split(";")[0]]
    assert len(lines) == 4 * 6, lines
    for width, n_per_policy in (("short", 1), ("dword ", 2), ("dwordx2", 1), ("dwordx4", 2)):
        assert sum(("_store_" + width) in ln + " " for ln in lines) == 4 * n_per_policy, (width, lines)
    through = [ln for ln in lines if " sc1" in ln]; streaming = [ln for ln in lines if ln.rstrip().endswith(" nt") or " nt " in ln]
    assert len(through) == 2 * 6 and len(streaming) == 2 * 6 and len([ln for ln in through if ln in streaming]) == 6, lines


def test_every_buffer_policy_can_be_overridden(tmp_path):
    """Every MON_SP_<buffer> constant takes a -D, and MON_SP_ALL reaches all of them (what the plain-store variant of the GPU test relies on)."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    names = ["E", "DE", "XSOA", "DW", "RAYOUT", "GPART", "HALF", "TILES", "EMA", "XALL", "FRAG", "STATE"]
    body = "#include \"store_policy.h\"\n" + "".join("static_assert(MON_SP_%s == WANT_%s, \"%s\");\n" % (n, n, n) for n in names)
    src = tmp_path / "pol.hip"; src.write_text(body)
    def compiles(defs, want):
        cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "-I", CSRC, "--cuda-device-only", "-fsyntax-only", str(src)] + defs
        cmd += ["-DWANT_%s=%s" % (n, want(n)) for n in names]
        return subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    assert compiles(["-DMON_SP_ALL=MON_SP_PLAIN"], lambda n: "MON_SP_PLAIN")
    assert compiles(["-DMON_SP_HANDOVER=MON_SP_WT"], lambda n: "MON_SP_NT" if n == "STATE" else "MON_SP_WT")
    for one in names:
        assert compiles(["-DMON_SP_ALL=MON_SP_PLAIN", "-DMON_SP_%s=MON_SP_WT_NT" % one], lambda n: "MON_SP_WT_NT" if n == one else "MON_SP_PLAIN"), one
    assert not compiles(["-DMON_SP_ALL=MON_SP_PLAIN"], lambda n: "MON_SP_WT")          # (the probe itself can fail)


FUSED_TILES = dict(rays_per_batch=1024, n_levels=16, n_neurons=64, n_hidden_layers=1)      # base.json's network: the level-tile chain of the fused backend


@pytest.mark.gpu
def test_skipped_batch_leaves_everything_untouched(pkg, ss, small_scene):
    """An object whose 3-D box no camera looks at: every candidate ray misses it, n_valid == 0, the iteration is skipped.  After a few real steps (so that
    every array holds live values) the skipped ones must leave master / fp16 copy / EMA / Adam moments / step counters bit-identical, count in
    skipped_batches and not advance the optimizer step; training the same object on real rays afterwards still works."""
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    sc = small_scene; ob = sc.objects[0]
    ds, obj = ge.make_problem(pkg, sc, FUSED_TILES)
    assert obj.info().backend == 1
    obj.train(4); trained = obj.get_params(0)
    cfg = pkg.default_config(**FUSED_TILES)
    far = ob["Tow"].copy(); far[:3, 3] += 50.0
    o2 = pkg.ObjectNeRF(ds, cfg, ob["cls"], ss.colmajor(far), -ob["half"], ob["half"]); o2.add_boxes(ob["boxes"])
    assert o2.info().backend == 1
    o2.set_params(trained)                                  # live weights; the moments / counters stay at their initial values, which must not move either
    names = ("master", "half", "ema", "m1", "m2", "steps")
    before = {n: o2.buffer(n).copy() for n in names}; p_before = [o2.get_params(w).copy() for w in (0, 1, 2)]
    step0 = o2.info().train_step
    o2.train(5)
    i = o2.info(); st = o2.buffer("state")
    assert i.skipped_batches == 5 and i.last_n_valid == 0 and int(st[7]) == 5 and i.train_step == step0
    for n in names:
        assert np.array_equal(before[n], o2.buffer(n)), n
    for w in (0, 1, 2):
        assert np.array_equal(p_before[w], o2.get_params(w)), w
    # the first object is unaffected by its neighbour's skipped launches and goes on learning
    l0 = obj.train(20); l1 = obj.train(60)
    assert obj.info().skipped_batches == 0 and np.isfinite(l1) and l1 < l0
    o2.close(); obj.close(); ds.close()


CRC_SCRIPT = """
import json, sys, zlib
sys.path.insert(0, %r)
import __graft_entry__ as ge
pkg = ge.load_package(); ss = ge.load_tools()
sc = ss.make_scene(n_views=40, H=480, W=640, f=525.0, seed=0)
ds, obj = ge.make_problem(pkg, sc, dict(sample_seed=2024))
out = {"lib": pkg.lib_path()}; done = 0
for upto in (25, 220):
    obj.train(upto - done); done = upto
    out[str(upto)] = ["%%08x" %% zlib.crc32(obj.get_params(w).tobytes()) for w in (0, 1, 2)] + ["%%08x" %% zlib.crc32(obj.buffer(n).tobytes()) for n in ("m1", "m2")]
print(json.dumps(out))
""" % ROOT


def _crcs(lib_path):
    env = dict(os.environ); env.pop("MON_CORE_LIB", None)
    if lib_path:
        env["MON_CORE_LIB"] = lib_path
    r = subprocess.run([sys.executable, "-c", CRC_SCRIPT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_policies_do_not_change_the_trained_parameters(pkg):
    """The bench object (bench.py's scene, seed and base.json network) after 25 and after 220 steps: master, fp16 copy, EMA and both Adam moments have the
    same CRC with the shipped library and with a tools/variant_build.sh build of the same sources whose every policy is plain (-DMON_SP_ALL=MON_SP_PLAIN)."""
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    tag = "sp_plain"; variant = os.path.join(ROOT, "ro-map_amd", "build_" + tag, "libmon_core.so")
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(variant) or any(os.path.getmtime(s) > os.path.getmtime(variant) for s in srcs):
        if not (os.path.exists(HIPCC) and shutil.which("bash")):
            pytest.skip("the plain-store variant cannot be built here: no hipcc")
        b = subprocess.run(["bash", os.path.join(ROOT, "tools", "variant_build.sh"), tag, "-DMON_SP_ALL=MON_SP_PLAIN"], stdout=subprocess.PIPE,
                stderr=subprocess.STDOUT, text=True)
        if b.returncode != 0 or not os.path.exists(variant):
            pytest.skip("the plain-store variant cannot be built here: %s" % b.stdout[-400:])
    shipped = _crcs(None); plain = _crcs(variant)
    assert os.path.samefile(plain["lib"], variant) and not os.path.samefile(shipped["lib"], variant)
    print("shipped", shipped); print("plain  ", plain)
    for upto in ("25", "220"):
        assert shipped[upto] == plain[upto], (upto, shipped[upto], plain[upto])
