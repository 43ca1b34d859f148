// checkpoint.cpp -- mon_object_save / mon_object_load / mon_checkpoint_read_info
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <unistd.h>
#include <zlib.h>
#include "model_internal.h"
#include "xorwow.h"

namespace mon {
// ------------------------------------------------------------------ checkpoints
// One object per file, little-endian, every field written one by one (never a struct image):
//   [0, 64)      header: magic "MONCKPT\0", version, section count, file bytes, table offset, CRC-32 of [0, table end) with the CRC field as zero
//   [64, 320)    object block: every mon_config field, class id, Tow, box, parameter counts, backend, step-counter width, lazy-EMA and occupancy flags, box count
//   [320, 448)   state block: what the next iteration and mon_object_info_get read (DevState's head as words, the occupancy schedule, the pending-EMA flag)
//   [448, ..)    section table, 32 bytes per entry: tag[8], element type, CRC-32 of the section, element count, byte offset (a multiple of 64)
// then the sections, each a flat array in parameter order whatever the layout in device memory (arrays or 128-byte chunk records).
static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the checkpoint writer stores host words as they are");
namespace {
constexpr char kCkMagic[8] = { 'M', 'O', 'N', 'C', 'K', 'P', 'T', 0 };
constexpr uint32_t kCkVersion = 1, kCkHeaderBytes = 64, kCkObjectOff = 64, kCkStateOff = 320, kCkTableOff = 448, kCkEntryBytes = 32, kCkMaxSections = 16;
// the one pinned and the one device staging buffer of a save / load: never more than this, whatever the table size
constexpr size_t kCkStageBytes = (size_t)32 << 20;
enum { CK_F32 = 1, CK_U32 = 2, CK_F16 = 3, CK_BBOX = 4 };
constexpr size_t ck_elem_bytes(uint32_t type) { return type == CK_F16 ? 2 : type == CK_BBOX ? 20 : 4; }
// state block words
enum { CKS_STEP = 0, CKS_ITER, CKS_SKIPPED, CKS_LR, CKS_N_VALID, CKS_LOSS_SUM, CKS_N_VALID_PRE, CKS_SCATTER_NOW, CKS_SCATTER_LAST, CKS_SCATTER_TOTAL,
       CKS_DEB_OLD, CKS_DEB_NEW, CKS_DEB_EVEN_OLD, CKS_DEB_EVEN_NEW, CKS_OCC_REFRESHED, CKS_OCC_NEXT, CKS_OCC_THRESHOLD, CKS_EMA_PENDING, CKS_WORDS = 32 };
struct CkSection { std::string tag; uint32_t type = 0, crc = 0; uint64_t count = 0, offset = 0; size_t bytes() const { return (size_t)count * ck_elem_bytes(type); } };
struct CkFile { mon_checkpoint_info info{}; uint32_t step_bits = 0, state[CKS_WORDS] = {}; std::vector<CkSection> sec;
    const CkSection* find(const char* tag) const { for (const CkSection& s : sec) if (s.tag == tag) return &s; return nullptr; } };

void put32(uint8_t* b, size_t off, uint32_t v) { std::memcpy(b + off, &v, 4); }
void put64(uint8_t* b, size_t off, uint64_t v) { std::memcpy(b + off, &v, 8); }
void putf(uint8_t* b, size_t off, float v) { std::memcpy(b + off, &v, 4); }
uint32_t get32(const uint8_t* b, size_t off) { uint32_t v; std::memcpy(&v, b + off, 4); return v; }
uint64_t get64(const uint8_t* b, size_t off) { uint64_t v; std::memcpy(&v, b + off, 8); return v; }
float getf(const uint8_t* b, size_t off) { float v; std::memcpy(&v, b + off, 4); return v; }
uint32_t f2u(float f) { uint32_t v; std::memcpy(&v, &f, 4); return v; }
float u2f(uint32_t u) { float v; std::memcpy(&v, &u, 4); return v; }
uint32_t ck_crc(uint32_t crc, const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    while (n) { const size_t k = n < ((size_t)1 << 30) ? n : ((size_t)1 << 30); crc = (uint32_t)::crc32(crc, b, (uInt)k); b += k; n -= k; }
    return crc;
}

// the sections a file of this object block holds, in file order
std::vector<CkSection> ck_expected_sections(const mon_checkpoint_info& in) {
    std::vector<CkSection> v; const uint64_t n = in.n_params;
    auto add = [&](const char* tag, uint32_t type, uint64_t count) { CkSection s; s.tag = tag; s.type = type; s.count = count; v.push_back(s); };
    add("master", CK_F32, n); add("m1", CK_F32, n); add("m2", CK_F32, n); add("steps", CK_U32, n); add("ema", CK_F16, n);
    if (in.lazy_ema) add("ema_step", CK_U32, n >> 3);
    if (in.has_occupancy) { add("occ", CK_U32, kOccWords); add("occ_raw", CK_U32, kOccWords); }
    add("boxes", CK_BBOX, in.n_boxes);
    return v;
}
void ck_layout(std::vector<CkSection>& sec, uint64_t* file_bytes) {
    uint64_t off = kCkTableOff + (uint64_t)kCkEntryBytes * sec.size();
    for (CkSection& s : sec) { off = (off + 63u) & ~(uint64_t)63u; s.offset = off; off += s.bytes(); }
    *file_bytes = off;
}
// header + object block + state block + table, CRC included
std::vector<uint8_t> ck_head_bytes(const CkFile& ck) {
    const mon_checkpoint_info& in = ck.info; const mon_config& c = in.cfg;
    std::vector<uint8_t> h(kCkTableOff + (size_t)kCkEntryBytes * ck.sec.size(), 0); uint8_t* b = h.data();
    std::memcpy(b, kCkMagic, 8); put32(b, 8, kCkVersion); put32(b, 12, (uint32_t)ck.sec.size()); put64(b, 16, in.file_bytes); put32(b, 24, kCkTableOff);
    size_t o = kCkObjectOff;
    put32(b, o, (uint32_t)c.n_levels); put32(b, o + 4, (uint32_t)c.n_features); put32(b, o + 8, (uint32_t)c.log2_hashmap_size);
    put32(b, o + 12, (uint32_t)c.base_resolution); putf(b, o + 16, c.per_level_scale); put32(b, o + 20, (uint32_t)c.n_neurons);
    put32(b, o + 24, (uint32_t)c.n_hidden_layers); put32(b, o + 28, (uint32_t)c.rays_per_batch); put32(b, o + 32, (uint32_t)c.n_samples);
    putf(b, o + 36, c.loss_scale); putf(b, o + 40, c.learning_rate); putf(b, o + 44, c.beta1); putf(b, o + 48, c.beta2); putf(b, o + 52, c.epsilon);
    putf(b, o + 56, c.l2_reg); putf(b, o + 60, c.ema_decay); put32(b, o + 64, (uint32_t)c.decay_start); put32(b, o + 68, (uint32_t)c.decay_interval);
    putf(b, o + 72, c.decay_base); put32(b, o + 76, c.param_seed); put32(b, o + 80, c.rng_flags); put32(b, o + 84, (uint32_t)c.use_depth);
    put32(b, o + 88, (uint32_t)c.occupancy_skip); put32(b, o + 92, 0u); put64(b, o + 96, c.sample_seed);
    put32(b, o + 104, (uint32_t)in.class_id);
    for (int i = 0; i < 16; ++i) putf(b, o + 108 + 4 * i, in.Tow[i]);
    for (int i = 0; i < 3; ++i) { putf(b, o + 172 + 4 * i, in.aabb_min[i]); putf(b, o + 184 + 4 * i, in.aabb_max[i]); }
    put32(b, o + 196, in.n_params); put32(b, o + 200, in.n_mlp_params); put32(b, o + 204, in.n_grid_params); put32(b, o + 208, (uint32_t)in.backend);
    put32(b, o + 212, ck.step_bits); put32(b, o + 216, in.lazy_ema); put32(b, o + 220, in.has_occupancy); put32(b, o + 224, in.n_boxes);
    for (uint32_t i = 0; i < CKS_WORDS; ++i) put32(b, kCkStateOff + 4 * i, ck.state[i]);
    for (size_t k = 0; k < ck.sec.size(); ++k) {
        const CkSection& s = ck.sec[k]; const size_t e = kCkTableOff + kCkEntryBytes * k;
        std::memcpy(b + e, s.tag.data(), std::min<size_t>(s.tag.size(), 8)); put32(b, e + 8, s.type); put32(b, e + 12, s.crc); put64(b, e + 16, s.count);
        put64(b, e + 24, s.offset);
    }
    put32(b, 28, ck_crc(0u, b, h.size()));
    return h;
}

struct FileCloser { FILE* f = nullptr; ~FileCloser() { if (f) std::fclose(f); } };

// Everything that can be judged without a device: MON_ERR_IO with a message, or the parsed head.
int ck_parse(FILE* f, const char* path, CkFile& ck) {
#define CK_BAD(...) do { set_error(__VA_ARGS__); return MON_ERR_IO; } while (0)
    if (std::fseek(f, 0, SEEK_END) != 0) CK_BAD("checkpoint %s: cannot seek", path);
    const long flen = std::ftell(f);
    if (flen < (long)kCkHeaderBytes) CK_BAD("checkpoint %s: truncated (%ld bytes, the header alone is %u)", path, flen, kCkHeaderBytes);
    uint8_t hd[kCkHeaderBytes];
    if (std::fseek(f, 0, SEEK_SET) != 0 || std::fread(hd, 1, kCkHeaderBytes, f) != kCkHeaderBytes) CK_BAD("checkpoint %s: cannot read the header", path);
    if (std::memcmp(hd, kCkMagic, 8) != 0) CK_BAD("checkpoint %s: bad magic", path);
    const uint32_t version = get32(hd, 8), n_sec = get32(hd, 12);
    if (version == 0u || version > kCkVersion) CK_BAD("checkpoint %s: format version %u, this build reads up to %u", path, version, kCkVersion);
    if (n_sec > kCkMaxSections || get32(hd, 24) != kCkTableOff) CK_BAD("checkpoint %s: %u sections / table offset %u", path, n_sec, get32(hd, 24));
    const uint64_t file_bytes = get64(hd, 16); const size_t head_len = kCkTableOff + (size_t)kCkEntryBytes * n_sec;
    if (file_bytes != (uint64_t)flen) CK_BAD("checkpoint %s: truncated or extended (%ld bytes, the header says %llu)", path, flen,
            (unsigned long long)file_bytes);
    if ((uint64_t)head_len > file_bytes) CK_BAD("checkpoint %s: truncated inside the section table", path);
    std::vector<uint8_t> h(head_len);
    if (std::fseek(f, 0, SEEK_SET) != 0 || std::fread(h.data(), 1, head_len, f) != head_len) CK_BAD("checkpoint %s: cannot read the section table", path);
    const uint8_t* b = h.data();
    { const uint32_t stored = get32(b, 28); put32(h.data(), 28, 0u);
      if (ck_crc(0u, b, head_len) != stored) CK_BAD("checkpoint %s: header / section table CRC mismatch", path); }
    mon_checkpoint_info& in = ck.info; mon_config& c = in.cfg; size_t o = kCkObjectOff;
    in.version = version; in.file_bytes = file_bytes;
    c.n_levels = (int32_t)get32(b, o); c.n_features = (int32_t)get32(b, o + 4); c.log2_hashmap_size = (int32_t)get32(b, o + 8);
    c.base_resolution = (int32_t)get32(b, o + 12); c.per_level_scale = getf(b, o + 16); c.n_neurons = (int32_t)get32(b, o + 20);
    c.n_hidden_layers = (int32_t)get32(b, o + 24); c.rays_per_batch = (int32_t)get32(b, o + 28); c.n_samples = (int32_t)get32(b, o + 32);
    c.loss_scale = getf(b, o + 36); c.learning_rate = getf(b, o + 40); c.beta1 = getf(b, o + 44); c.beta2 = getf(b, o + 48); c.epsilon = getf(b, o + 52);
    c.l2_reg = getf(b, o + 56); c.ema_decay = getf(b, o + 60); c.decay_start = (int32_t)get32(b, o + 64); c.decay_interval = (int32_t)get32(b, o + 68);
    c.decay_base = getf(b, o + 72); c.param_seed = get32(b, o + 76); c.rng_flags = get32(b, o + 80); c.use_depth = (int32_t)get32(b, o + 84);
    c.occupancy_skip = (int32_t)get32(b, o + 88); c.sample_seed = get64(b, o + 96);
    in.class_id = (int32_t)get32(b, o + 104);
    for (int i = 0; i < 16; ++i) in.Tow[i] = getf(b, o + 108 + 4 * i);
    for (int i = 0; i < 3; ++i) { in.aabb_min[i] = getf(b, o + 172 + 4 * i); in.aabb_max[i] = getf(b, o + 184 + 4 * i); }
    in.n_params = get32(b, o + 196); in.n_mlp_params = get32(b, o + 200); in.n_grid_params = get32(b, o + 204); in.backend = (int32_t)get32(b, o + 208);
    ck.step_bits = get32(b, o + 212); in.lazy_ema = get32(b, o + 216); in.has_occupancy = get32(b, o + 220); in.n_boxes = get32(b, o + 224);
    for (uint32_t i = 0; i < CKS_WORDS; ++i) ck.state[i] = get32(b, kCkStateOff + 4 * i);
    in.train_step = ck.state[CKS_STEP]; in.iter = ck.state[CKS_ITER];
    // the config, through mon_object_create's checks (their messages stand), and the sizes it implies
    if (config_check(c) != MON_OK) return MON_ERR_IO;
    if (rng_stream_mode(c.rng_flags)) CK_BAD("checkpoint %s: an object in the XORWOW sample-stream mode (not a checkpoint this library writes)", path);
    LevelTable lt{}; NetDims nd{}; uint32_t n_grid = 0;
    if (level_table_build(c, lt, nd, n_grid) != MON_OK) return MON_ERR_IO;
    if (in.n_mlp_params != (uint32_t)nd.n_mlp || in.n_grid_params != n_grid || in.n_params != (uint32_t)nd.n_mlp + n_grid || (in.n_params & 7u) != 0u)
        CK_BAD("checkpoint %s: %u = %u + %u parameters, its config has %u + %u", path, in.n_params, in.n_mlp_params, in.n_grid_params, (uint32_t)nd.n_mlp,
                n_grid);
    if (ck.step_bits != 16u && ck.step_bits != 32u) CK_BAD("checkpoint %s: step counters of %u bits", path, ck.step_bits);
    if (in.lazy_ema > 1u || in.has_occupancy > 1u || (in.lazy_ema != 0u) != (n_grid > (8u << 20)) || (in.has_occupancy && !c.occupancy_skip))
        CK_BAD("checkpoint %s: lazy-EMA / occupancy flags %u / %u do not fit its config", path, in.lazy_ema, in.has_occupancy);
    if ((in.backend != 0 && in.backend != 1) || (in.backend == 1 && !fused_supported(nd, (uint32_t)c.n_samples, (uint32_t)c.rays_per_batch)))
        CK_BAD("checkpoint %s: backend %d for this network shape", path, in.backend);
    // the section table against what this object block implies
    std::vector<CkSection> want = ck_expected_sections(in);
    if (want.size() != n_sec) CK_BAD("checkpoint %s: %u sections, its object block implies %zu", path, n_sec, want.size());
    ck.sec.clear();
    for (uint32_t k = 0; k < n_sec; ++k) {
        const size_t e = kCkTableOff + (size_t)kCkEntryBytes * k; CkSection s; char tag[9] = {}; std::memcpy(tag, b + e, 8); s.tag = tag;
        s.type = get32(b, e + 8); s.crc = get32(b, e + 12); s.count = get64(b, e + 16); s.offset = get64(b, e + 24);
        const CkSection* w = nullptr; for (const CkSection& q : want) if (q.tag == s.tag) w = &q;
        if (!w || ck.find(tag)) CK_BAD("checkpoint %s: unexpected or repeated section \"%s\"", path, tag);
        if (s.type != w->type || s.count != w->count) CK_BAD("checkpoint %s: section \"%s\" holds %llu elements of type %u, expected %llu of type %u", path, tag,
                (unsigned long long)s.count, s.type, (unsigned long long)w->count, w->type);
        if ((s.offset & 63u) != 0u || s.offset < head_len || s.offset > file_bytes || s.bytes() > file_bytes - s.offset)
            CK_BAD("checkpoint %s: section \"%s\" at offset %llu (%zu bytes) does not lie inside the file's %llu bytes", path, tag,
                    (unsigned long long)s.offset, s.bytes(), (unsigned long long)file_bytes);
        // (no two sections share a byte: what lies between them is padding only)
        for (const CkSection& q : ck.sec) if (s.offset < q.offset + q.bytes() && q.offset < s.offset + s.bytes())
            CK_BAD("checkpoint %s: sections \"%s\" and \"%s\" overlap", path, q.tag.c_str(), tag);
        ck.sec.push_back(s);
    }
    return MON_OK;
}
int ck_verify_sections(FILE* f, const char* path, const CkFile& ck) {
    std::vector<uint8_t> buf((size_t)1 << 20);
    for (const CkSection& s : ck.sec) {
        if (std::fseek(f, (long)s.offset, SEEK_SET) != 0) CK_BAD("checkpoint %s: cannot seek to section \"%s\"", path, s.tag.c_str());
        uint32_t crc = 0u;
        for (size_t left = s.bytes(); left; ) { const size_t k = std::min(left, buf.size());
            if (std::fread(buf.data(), 1, k, f) != k) CK_BAD("checkpoint %s: cannot read section \"%s\"", path, s.tag.c_str());
            crc = ck_crc(crc, buf.data(), k); left -= k; }
        if (crc != s.crc) CK_BAD("checkpoint %s: CRC mismatch in section \"%s\"", path, s.tag.c_str());
    }
    return MON_OK;
}

std::atomic<int> g_ck_timing{ 0 }; thread_local double g_ck_kernel_ms = 0.0;
// the bounded staging of one save / load; everything is released when it goes out of scope
struct CkStage {
    uint8_t* h = nullptr; uint8_t* d = nullptr; size_t cap = 0; hipEvent_t e0 = nullptr, e1 = nullptr; bool timed = false, pending = false;
    int init(size_t largest_section, bool need_device) {
        cap = std::max<size_t>(std::min(kCkStageBytes, largest_section), 64); cap = (cap + 63) & ~(size_t)63;
        HIPCHECK(hipHostMalloc((void**)&h, cap, hipHostMallocDefault));
        if (need_device) HIPCHECK(hipMalloc((void**)&d, cap));
        timed = g_ck_timing.load() != 0;
        if (timed) { HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1)); }
        return MON_OK;
    }
    void before_kernel(hipStream_t s) { if (timed) { (void)hipEventRecord(e0, s); pending = true; } }
    void after_kernel(hipStream_t s) { if (timed) (void)hipEventRecord(e1, s); }
    // (after the stream has been synchronised)
    void collect() { if (pending) { float ms = 0.f; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) g_ck_kernel_ms += ms; pending = false; } }
    ~CkStage() { if (h) (void)hipHostFree(h); if (d) (void)hipFree(d); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
// where a section lives in this build's device memory: a plain array (`direct`), or something a kernel converts range by range
struct CkDevSection { void* direct = nullptr; int rec_which = -1; bool steps16 = false; };
CkDevSection ck_dev_section(Model& m, const std::string& tag) {
    CkDevSection s;
    if (tag == "ema") s.direct = m.P.ema;
    else if (tag == "occ") s.direct = m.d_occ;
    else if (tag == "occ_raw") s.direct = m.d_occ_tmp;
    else if (tag == "boxes") s.direct = m.d_boxes;
    else if (tag == "ema_step") { if (m.P.rec) s.rec_which = 4; else s.direct = m.d_ema_step; }
    else if (tag == "steps") { if (m.P.rec) s.rec_which = 3; else if (m.P.steps16) s.steps16 = true; else s.direct = m.P.steps; }
    else if (m.P.rec) s.rec_which = tag == "master" ? 0 : tag == "m1" ? 1 : 2;
    else s.direct = tag == "master" ? (void*)m.P.master : tag == "m1" ? (void*)m.P.m1 : (void*)m.P.m2;
    return s;
}
}  // namespace

int checkpoint_timing(int enable, double* kernel_ms) {
    g_ck_timing.store(enable ? 1 : 0); if (kernel_ms) *kernel_ms = g_ck_kernel_ms; g_ck_kernel_ms = 0.0; return MON_OK;
}

int checkpoint_read_info(const char* path, int verify, mon_checkpoint_info* out) {
    if (!path || !out) { set_error("checkpoint_read_info: null argument"); return MON_ERR_ARG; }
    FileCloser fc; fc.f = std::fopen(path, "rb");
    if (!fc.f) { set_error("checkpoint %s: cannot open", path); return MON_ERR_IO; }
    CkFile ck; int rc = ck_parse(fc.f, path, ck); if (rc) return rc;
    if (verify && (rc = ck_verify_sections(fc.f, path, ck))) return rc;
    *out = ck.info; return MON_OK;
}

int model_save(Model& m, const char* path) {
    if (!path) { set_error("object_save: null path"); return MON_ERR_ARG; }
    if (m.d_xw) { set_error("object_save: an object in the XORWOW sample-stream mode (its generator state is not stored)"); return MON_ERR_STATE; }
    if (m.scatter_pending) { set_error("object_save: between the stages of an iteration (mon_object_train_stages)"); return MON_ERR_STATE; }
    if (m.n_params & 7u) { set_error("object_save: %u parameters (not whole chunks of 8)", m.n_params); return MON_ERR_STATE; }
    HIPCHECK(use_device(m.device)); model_leave_lane(m); HIPCHECK(hipStreamSynchronize(m.train_stream));
    hipStream_t s = m.train_stream;
    CkFile ck; mon_checkpoint_info& in = ck.info;
    in.version = kCkVersion; in.cfg = m.cfg; in.class_id = (int32_t)m.oc.instance_id; std::memcpy(in.Tow, m.oc.Tow.m, 64);
    for (int a = 0; a < 3; ++a) { in.aabb_min[a] = m.oc.aabb.mn[a]; in.aabb_max[a] = m.oc.aabb.mx[a]; }
    in.n_params = m.n_params; in.n_mlp_params = (uint32_t)m.nd.n_mlp; in.n_grid_params = m.n_grid; in.train_step = m.h_state.step; in.iter = m.h_state.iter;
    in.n_boxes = m.n_boxes; in.backend = m.backend; in.has_occupancy = (m.d_occ && m.occ_refreshed_iter) ? 1u : 0u; in.lazy_ema = m.plan.lazy_ema ? 1u : 0u;
    ck.step_bits = (m.P.rec || m.P.steps16) ? 16u : 32u;
    const DevState& st = m.h_state; uint32_t* w = ck.state;
    w[CKS_STEP] = st.step; w[CKS_ITER] = st.iter; w[CKS_SKIPPED] = st.skipped; w[CKS_LR] = f2u(st.lr); w[CKS_N_VALID] = st.n_valid;
    w[CKS_LOSS_SUM] = f2u(st.loss_sum); w[CKS_N_VALID_PRE] = st.n_valid_pre; w[CKS_SCATTER_NOW] = st.n_scatter_now; w[CKS_SCATTER_LAST] = st.n_scatter_last;
    w[CKS_SCATTER_TOTAL] = st.n_scatter_total; w[CKS_DEB_OLD] = f2u(st.ema_deb_old); w[CKS_DEB_NEW] = f2u(st.ema_deb_new);
    w[CKS_DEB_EVEN_OLD] = f2u(st.ema_deb_even_old); w[CKS_DEB_EVEN_NEW] = f2u(st.ema_deb_even_new); w[CKS_OCC_REFRESHED] = m.occ_refreshed_iter;
    w[CKS_OCC_NEXT] = m.occ_next_refresh; w[CKS_OCC_THRESHOLD] = f2u(m.occ_raw_threshold); w[CKS_EMA_PENDING] = m.ema_pending ? 1u : 0u;
    ck.sec = ck_expected_sections(in); { uint64_t fb = 0; ck_layout(ck.sec, &fb); in.file_bytes = fb; }
    size_t largest = 0; bool need_device = false;
    for (const CkSection& q : ck.sec) { largest = std::max(largest, q.bytes()); const CkDevSection dv = ck_dev_section(m, q.tag); need_device |= !dv.direct; }
    CkStage stage; { const int rc = stage.init(largest, need_device); if (rc) return rc; }

    const std::string tmp = std::string(path) + ".tmp";
    struct TmpFile { FileCloser fc; std::string name; bool keep = false; ~TmpFile() { if (fc.f) { std::fclose(fc.f); fc.f = nullptr; } if (!keep) std::remove(name.c_str()); } } out;
    out.name = tmp; out.fc.f = std::fopen(tmp.c_str(), "wb");
    if (!out.fc.f) { out.keep = true; set_error("object_save: cannot create %s", tmp.c_str()); return MON_ERR_IO; }
    FILE* f = out.fc.f;
#define CK_WRITE(ptr, n) do { if ((n) && std::fwrite((ptr), 1, (n), f) != (size_t)(n)) { set_error("object_save: write to %s failed", tmp.c_str()); \
        return MON_ERR_IO; } } while (0)
    uint64_t pos = 0; const std::vector<uint8_t> zeros(64, 0);
    { const std::vector<uint8_t> head(kCkTableOff + (size_t)kCkEntryBytes * ck.sec.size(), 0); CK_WRITE(head.data(), head.size()); pos = head.size(); }
    for (CkSection& q : ck.sec) {
        CK_WRITE(zeros.data(), (size_t)(q.offset - pos)); pos = q.offset;
        const CkDevSection dv = ck_dev_section(m, q.tag); const size_t total = q.bytes(); uint32_t crc = 0u;
        for (size_t off = 0; off < total; off += stage.cap) {
            const size_t n = std::min(stage.cap, total - off);
            if (dv.direct) HIPCHECK(hipMemcpyAsync(stage.h, static_cast<const uint8_t*>(dv.direct) + off, n, hipMemcpyDeviceToHost, s));
            else {
                // (whole chunks: every section of a converted kind is 4 or 32 bytes per chunk, and the staging size is a multiple of both)
                const size_t per_chunk = dv.rec_which == 4 ? 4 : 32; const uint32_t c0 = (uint32_t)(off / per_chunk), nc = (uint32_t)(n / per_chunk);
                stage.before_kernel(s);
                if (dv.steps16) launch_steps16_unpack_range(s, m.P.steps16, stage.d, c0, nc);
                else launch_state_unpack_range(s, m.P.rec, dv.rec_which, stage.d, c0, nc);
                stage.after_kernel(s);
                HIPCHECK(hipMemcpyAsync(stage.h, stage.d, n, hipMemcpyDeviceToHost, s));
            }
            HIPCHECK(hipStreamSynchronize(s)); stage.collect();
            crc = ck_crc(crc, stage.h, n); CK_WRITE(stage.h, n);
        }
        q.crc = crc; pos += total;
    }
    HIPCHECK(hipGetLastError());
    const std::vector<uint8_t> head = ck_head_bytes(ck);
    if (std::fseek(f, 0, SEEK_SET) != 0) { set_error("object_save: cannot seek in %s", tmp.c_str()); return MON_ERR_IO; }
    CK_WRITE(head.data(), head.size());
#undef CK_WRITE
    if (std::fflush(f) != 0 || ::fsync(::fileno(f)) != 0) { set_error("object_save: flushing %s failed", tmp.c_str()); return MON_ERR_IO; }
    { const int crc_close = std::fclose(f); out.fc.f = nullptr; if (crc_close != 0) { set_error("object_save: closing %s failed", tmp.c_str()); return MON_ERR_IO; } }
    if (std::rename(tmp.c_str(), path) != 0) { set_error("object_save: cannot rename %s to %s", tmp.c_str(), path); return MON_ERR_IO; }
    out.keep = true;
    return MON_OK;
}

int model_load(Dataset* ds, const char* path, uint32_t flags, Model** out, std::vector<mon_frame_bbox>* boxes_out) {
    if (out) *out = nullptr;
    if (!ds || !path || !out) { set_error("object_load: null argument"); return MON_ERR_ARG; }
    if (flags & ~MON_LOAD_BOXES) { set_error("object_load: unknown flag bits %#x", flags & ~MON_LOAD_BOXES); return MON_ERR_ARG; }
    FileCloser fc; fc.f = std::fopen(path, "rb");
    if (!fc.f) { set_error("checkpoint %s: cannot open", path); return MON_ERR_IO; }
    FILE* f = fc.f;
    CkFile ck; { const int rc = ck_parse(f, path, ck); if (rc) return rc; }
    const mon_checkpoint_info& in = ck.info;
    if (ck.step_bits != (steps16_exact(in.cfg) ? 16u : 32u)) {
        set_error("checkpoint %s: %u-bit step counters, this build keeps %u-bit ones for that config", path, ck.step_bits, steps16_exact(in.cfg) ? 16u : 32u);
        return MON_ERR_STATE; }
    // the box list (small): read, checked against its CRC and -- when it is to be restored -- against the dataset, all before any device work
    std::vector<mon_frame_bbox> boxes(in.n_boxes);
    {   const CkSection* q = ck.find("boxes");
        if (in.n_boxes) {
            std::vector<uint8_t> raw(q->bytes());
            if (std::fseek(f, (long)q->offset, SEEK_SET) != 0 || std::fread(raw.data(), 1, raw.size(), f) != raw.size()) {
                set_error("checkpoint %s: cannot read section \"boxes\"", path); return MON_ERR_IO; }
            if (ck_crc(0u, raw.data(), raw.size()) != q->crc) { set_error("checkpoint %s: CRC mismatch in section \"boxes\"", path); return MON_ERR_IO; }
            for (uint32_t i = 0; i < in.n_boxes; ++i) { const uint8_t* r = raw.data() + 20 * (size_t)i;
                boxes[i] = mon_frame_bbox{ get32(r, 0), get32(r, 4), get32(r, 8), get32(r, 12), get32(r, 16) }; }
        } else if (q->crc != 0u) { set_error("checkpoint %s: CRC mismatch in section \"boxes\"", path); return MON_ERR_IO; }
    }
    const bool with_boxes = (flags & MON_LOAD_BOXES) != 0u && in.n_boxes != 0u;
    if (with_boxes) for (uint32_t i = 0; i < in.n_boxes; ++i) {
        const mon_frame_bbox& b = boxes[i];
        if (b.FrameId >= ds->max_frames || !ds->present[b.FrameId]) {
            set_error("object_load: box %u names frame %u, which the dataset does not hold", i, b.FrameId); return MON_ERR_STATE; }
        if (b.w == 0 || b.h == 0 || b.x + b.w > (uint32_t)ds->K.W || b.y + b.h > (uint32_t)ds->K.H) {
            set_error("object_load: box %u (x %u y %u h %u w %u) outside the dataset's %dx%d images", i, b.x, b.y, b.h, b.w, ds->K.W, ds->K.H);
            return MON_ERR_STATE; }
    }
    if (boxes_out) *boxes_out = boxes;

    Model* mp = nullptr;
    { const int rc = model_create_impl(ds, in.cfg, in.class_id, in.Tow, in.aabb_min, in.aabb_max, false, &mp); if (rc) return rc; }
    struct Guard { Model* m; ~Guard() { if (m) model_destroy(m); } } guard{ mp };
    Model& m = *mp; hipStream_t s = m.train_stream;
    if ((m.plan.lazy_ema ? 1u : 0u) != in.lazy_ema || ((m.P.rec || m.P.steps16) ? 16u : 32u) != ck.step_bits) {
        set_error("checkpoint %s: lazy-EMA / step-counter mode differs from the object this build creates for its config", path); return MON_ERR_STATE; }
    size_t largest = 0; bool need_device = false;
    for (const CkSection& q : ck.sec) if (q.tag != "boxes") { largest = std::max(largest, q.bytes()); need_device |= !ck_dev_section(m, q.tag).direct; }
    CkStage stage; { const int rc = stage.init(largest, need_device); if (rc) return rc; }
    for (const CkSection& q : ck.sec) {
        if (q.tag == "boxes") continue;
        const CkDevSection dv = ck_dev_section(m, q.tag); const size_t total = q.bytes(); uint32_t crc = 0u;
        // (a grid in the file of an object that keeps none here -- a shape outside the fused kernels -- is checked and dropped)
        const bool drop = (q.tag == "occ" || q.tag == "occ_raw") && !m.d_occ;
        if (std::fseek(f, (long)q.offset, SEEK_SET) != 0) { set_error("checkpoint %s: cannot seek to section \"%s\"", path, q.tag.c_str()); return MON_ERR_IO; }
        for (size_t off = 0; off < total; off += stage.cap) {
            const size_t n = std::min(stage.cap, total - off);
            if (std::fread(stage.h, 1, n, f) != n) { set_error("checkpoint %s: cannot read section \"%s\"", path, q.tag.c_str()); return MON_ERR_IO; }
            crc = ck_crc(crc, stage.h, n);
            if (drop) continue;
            if (dv.direct) HIPCHECK(hipMemcpyAsync(static_cast<uint8_t*>(dv.direct) + off, stage.h, n, hipMemcpyHostToDevice, s));
            else {
                const size_t per_chunk = dv.rec_which == 4 ? 4 : 32; const uint32_t c0 = (uint32_t)(off / per_chunk), nc = (uint32_t)(n / per_chunk);
                HIPCHECK(hipMemcpyAsync(stage.d, stage.h, n, hipMemcpyHostToDevice, s));
                stage.before_kernel(s);
                if (dv.steps16) launch_steps16_pack_range(s, m.P.steps16, stage.d, c0, nc);
                else launch_state_pack_range(s, m.P.rec, dv.rec_which, stage.d, c0, nc);
                stage.after_kernel(s);
                // h(master) of the range while it sits in the staging buffer as a flat array (the records have no flat master to convert later)
                if (dv.rec_which == 0) launch_master_to_half(s, reinterpret_cast<const float*>(stage.d), m.P.half + 8u * (size_t)c0, 8u * nc);
            }
            HIPCHECK(hipStreamSynchronize(s)); stage.collect();             // (the staging buffers are reused by the next range)
        }
        if (crc != q.crc) { set_error("checkpoint %s: CRC mismatch in section \"%s\"", path, q.tag.c_str()); return MON_ERR_IO; }
        if (q.tag == "master" && dv.direct) launch_master_to_half(s, m.P.master, m.P.half, m.n_params);      // h(master), the rounding of every update
    }
    HIPCHECK(hipGetLastError()); HIPCHECK(hipStreamSynchronize(s));
    if (with_boxes) { const int rc = model_add_boxes(m, boxes.data(), boxes.size()); if (rc) return rc; }
    // the training state: both DevStates start as the saved one (iteration i reads one and writes everything that changes into the other; the slot counters
    // of both parities are clear between iterations)
    const uint32_t* w = ck.state;
    DevState st{}; st.step = w[CKS_STEP]; st.iter = w[CKS_ITER]; st.skipped = w[CKS_SKIPPED]; st.lr = u2f(w[CKS_LR]); st.n_valid = w[CKS_N_VALID];
    st.loss_sum = u2f(w[CKS_LOSS_SUM]); st.n_valid_pre = w[CKS_N_VALID_PRE]; st.n_scatter_now = w[CKS_SCATTER_NOW]; st.n_scatter_last = w[CKS_SCATTER_LAST];
    st.n_scatter_total = w[CKS_SCATTER_TOTAL]; st.ema_deb_old = u2f(w[CKS_DEB_OLD]); st.ema_deb_new = u2f(w[CKS_DEB_NEW]);
    st.ema_deb_even_old = u2f(w[CKS_DEB_EVEN_OLD]); st.ema_deb_even_new = u2f(w[CKS_DEB_EVEN_NEW]); st.n_boxes = m.n_boxes;
    m.h_state = st;
    HIPCHECK(hipMemcpy(m.d_state, &st, sizeof(DevState), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(m.d_state_next, &st, sizeof(DevState), hipMemcpyHostToDevice));
    if (m.d_occ && in.has_occupancy) { m.occ_refreshed_iter = w[CKS_OCC_REFRESHED]; m.occ_next_refresh = w[CKS_OCC_NEXT]; }
    if (m.d_occ) m.occ_raw_threshold = u2f(w[CKS_OCC_THRESHOLD]);
    m.ema_pending = m.plan.lazy_ema && w[CKS_EMA_PENDING] != 0u;
    m.backend = in.backend;
    // every derived image is rebuilt from the weights by the next iteration / render, as after set_params
    model_mark_stale(m, kStaleRays | kStaleWeights); m.scatter_pending = false;
    m.weights_epoch = next_weights_epoch();
    { const int rc = publish_snapshot(m); if (rc) return rc; }
    HIPCHECK(hipStreamSynchronize(nullptr)); HIPCHECK(hipStreamSynchronize(m.train_stream));
    guard.m = nullptr; *out = mp; return MON_OK;
#undef CK_BAD
}

}  // namespace mon
