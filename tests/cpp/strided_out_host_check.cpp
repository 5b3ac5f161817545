// strided_out_host_check -- the HOST side of emb_lookup_strided / emb_plan_create_strided (pimemb.h) against
// tests/cpp/hip_runtime_stub.cpp, for AddressSanitizer + UBSan: kernels are no-ops there and "device" memory is host memory, so
// what is checked is what the engine does around the launch -- the refusals, the grouping of mixed descriptors, plan text /
// signature / bytes, and what reaches the kernels: every launch of a bag kernel is looked at (the linker's --wrap puts the two
// functions below in front of the stub's hipLaunchKernel and __hipRegisterFunction) for its kernel's name and for word 3 of the
// view area of each of its descriptors (byte 112 of the 128-byte DevDesc: the row stride of a strided output), which must be
// the stride in a strided launch and zero in every other one -- dense, ranged, queue flush.  Linked with the library's host
// objects as tests/cpp/build_host_logic_check.sh builds them (tests/test_strided_out_cpu.py); nothing of this is linked into
// libpimemb.so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>
#include "pimemb.h"
#define CHECK(x) do { int rc_ = (x); if (rc_ != EMB_OK) { printf("FAIL %s:%d rc=%d %s\n", __FILE__, __LINE__, rc_, emb_last_error()); exit(1);} } while (0)
#define EXPECT(c) do { if (!(c)) { printf("EXPECT failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, emb_last_error()); exit(1);} } while (0)
// (the sharded call's RCCL binding is not linked: nothing here makes a shard)
extern "C" int emb_comm_rank(const emb_comm *, int32_t *, int32_t *) { return EMB_ERR_UNSUPPORTED; }
extern "C" int emb_comm_exchange(emb_comm *, const emb_comm_op *, uint32_t, void *) { return EMB_ERR_UNSUPPORTED; }

// ---- what the kernels are handed ---------------------------------------------------------------------------------------------
struct Dim3 { unsigned x, y, z; };            // (the layout of HIP's dim3, passed by value the same way)
struct Launch {
    std::string kernel;
    std::vector<uint64_t> stride_word;        // DevDesc::words[3] of every descriptor of the launch
};
static std::mutex g_mu;
static std::map<const void *, std::string> g_names;
static std::vector<Launch> g_launches;

extern "C" {
void __real___hipRegisterFunction(void **, const void *, char *, const char *, unsigned int, void *, void *, void *, void *, int *);
void __wrap___hipRegisterFunction(void **h, const void *host_fn, char *a, const char *device_name, unsigned int b, void *c, void *d, void *e,
                                  void *f, int *g) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_names[host_fn] = device_name ? device_name : "";
    }
    __real___hipRegisterFunction(h, host_fn, a, device_name, b, c, d, e, f, g);
}
int __real_hipLaunchKernel(const void *, Dim3, Dim3, void **, size_t, void *);
int __wrap_hipLaunchKernel(const void *fn, Dim3 grid, Dim3 block, void **args, size_t shmem, void *stream) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_names.find(fn);
        // the bag kernels: (const DevDesc *descs, uint32_t chunks, const uint32_t *xmap); without an XCD map grid.y is the
        // number of descriptors (every launch of this program: lane-group launches and one-descriptor wave-batch ones)
        if (it != g_names.end() && it->second.find("_kernel") != std::string::npos && it->second.find("6pimemb") != std::string::npos &&
            it->second.find("bag_") != std::string::npos) {
            Launch l;
            l.kernel = it->second;
            const char *descs = *static_cast<const char *const *>(args[0]);
            const bool mapped = l.kernel.find("anydim") == std::string::npos && l.kernel.find("hot") == std::string::npos &&
                                *static_cast<const void *const *>(args[2]) != nullptr;
            if (!mapped)
                for (unsigned i = 0; i < grid.y; i++) {
                    uint64_t w;
                    memcpy(&w, descs + 128 * (size_t)i + 112, 8);
                    l.stride_word.push_back(w);
                }
            g_launches.push_back(l);
        }
    }
    return __real_hipLaunchKernel(fn, grid, block, args, shmem, stream);
}
}

static std::vector<Launch> take_launches() {
    std::lock_guard<std::mutex> lk(g_mu);
    std::vector<Launch> out;
    out.swap(g_launches);
    return out;
}
static bool has(const std::string &s, const char *frag) { return s.find(frag) != std::string::npos; }
static size_t count(const std::string &s, const char *frag) {
    size_t n = 0, at = 0;
    while ((at = s.find(frag, at)) != std::string::npos) { n++; at++; }
    return n;
}

int main() {
    emb_config cfg{}; cfg.device = 0; cfg.max_tables = 8;
    emb_engine *e = nullptr; CHECK(emb_create(&cfg, &e));
    const uint32_t R = 100, B = 40, D = 16;
    std::vector<float> f32(R * D, 0.5f), f6(R * 6, 0.5f); std::vector<uint16_t> h16(R * D, 0x3f80); std::vector<int32_t> fx(R * D, 7);
    CHECK(emb_load_table(e, 0, R, D, EMB_F32, f32.data(), EMB_MEM_HOST));
    CHECK(emb_load_table(e, 1, R, D, EMB_BF16, h16.data(), EMB_MEM_HOST));
    CHECK(emb_load_table(e, 2, R, D, EMB_FIXED32, fx.data(), EMB_MEM_HOST));
    CHECK(emb_load_table(e, 3, R, 6, EMB_F32, f6.data(), EMB_MEM_HOST));
    CHECK(emb_load_table(e, 4, R, D, EMB_F16, h16.data(), EMB_MEM_HOST));
    std::vector<uint32_t> idx(B * 3), off(B);
    for (uint32_t b = 0; b < B; b++) off[b] = 3 * b;
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (uint32_t)(i * 7 % R);
    std::vector<float> w(idx.size(), 1.f);
    const uint64_t W = 4 + 4 * D + 8;                  // 4 leading columns, four tables' rows, a gap
    void *di, *dof, *dw, *dbuf, *down;
    CHECK(emb_device_alloc(e, idx.size() * 4, &di)); CHECK(emb_device_alloc(e, B * 4, &dof)); CHECK(emb_device_alloc(e, idx.size() * 4, &dw));
    CHECK(emb_device_alloc(e, B * W * 4, &dbuf)); CHECK(emb_device_alloc(e, B * D * 4, &down));       // EXACTLY sized
    CHECK(emb_copy_to_device(e, di, idx.data(), idx.size() * 4)); CHECK(emb_copy_to_device(e, dof, off.data(), B * 4));
    CHECK(emb_copy_to_device(e, dw, w.data(), idx.size() * 4));
    float *buf = static_cast<float *>(dbuf);
    auto desc = [&](uint32_t table, float *pooled) { return emb_lookup_desc{table, 0, di, dof, idx.size(), B, pooled}; };
    (void)take_launches();

    // ---- refusals: nothing is launched, emb_last_error names the descriptor, each UNSUPPORTED has words of its own -----------
    {
        std::set<std::string> texts;
        emb_plan *p = nullptr;
        auto both = [&](emb_lookup_desc d, const emb_pool_spec *ps, uint64_t stride, int want) {
            EXPECT(emb_lookup_strided(e, &d, ps, &stride, 1, EMB_IDX_U32, nullptr, 0, nullptr) == want);
            EXPECT(strstr(emb_last_error(), "desc 0") != nullptr);
            std::string t = emb_last_error();
            EXPECT(emb_plan_create_strided(e, &d, ps, &stride, 1, EMB_IDX_U32, &p) == want && p == nullptr);
            EXPECT(t == emb_last_error());
            if (want == EMB_ERR_UNSUPPORTED) texts.insert(t);
        };
        both(desc(0, buf), nullptr, 12, EMB_ERR_INVALID);                  // stride < dim
        both(desc(0, buf), nullptr, 18, EMB_ERR_INVALID);                  // stride % 4
        both(desc(0, buf), nullptr, 1ull << 32, EMB_ERR_INVALID);          // beyond 32 bits
        both(desc(0, buf + 2), nullptr, W, EMB_ERR_INVALID);               // pooled not 16-byte aligned
        both(desc(3, buf), nullptr, 8, EMB_ERR_UNSUPPORTED);               // a table on the any-dim kernels
        both(desc(2, buf), nullptr, W, EMB_ERR_UNSUPPORTED);               // fixed point
        emb_pool_spec half = {EMB_POOL_SUM, EMB_POOL_OUT_TABLE_DTYPE, nullptr, 0};
        both(desc(4, buf), &half, W, EMB_ERR_UNSUPPORTED);                 // half-width output with a stride
        EXPECT(texts.size() == 3);
        uint64_t st = W; emb_lookup_desc d0 = desc(0, buf);
        EXPECT(emb_lookup_strided(e, &d0, nullptr, &st, 1, EMB_IDX_U32, nullptr, 3, nullptr) == EMB_ERR_INVALID);     // check value
        EXPECT(take_launches().empty());
    }

    // ---- mixed descriptors: grouping, plan text, what reaches the kernels ----------------------------------------------------
    {
        // 0: fp32 dense (stride 0, a buffer of its own)   1, 2: fp32 strided   3: bf16 strided   4: fp32 strided, mean
        emb_lookup_desc d[5] = {desc(0, static_cast<float *>(down)), desc(0, buf + 4), desc(0, buf + 4 + D), desc(1, buf + 4 + 2 * D),
                                desc(0, buf + 4 + 3 * D)};
        emb_pool_spec ps[5] = {{EMB_POOL_SUM, 0, nullptr, 0}, {EMB_POOL_SUM, 0, nullptr, 0}, {EMB_POOL_SUM, 0, nullptr, 0},
                               {EMB_POOL_SUM, 0, nullptr, 0}, {EMB_POOL_MEAN, EMB_POOL_PADDING, nullptr, 3}};
        uint64_t st[5] = {0, W, W, W, W};
        emb_plan *p = nullptr; char text[4096];
        CHECK(emb_plan_create_strided(e, d, ps, st, 5, EMB_IDX_U32, &p));
        CHECK(emb_plan_describe(p, text, sizeof text)); printf("mixed: %s\n", text);
        std::string s(text);
        EXPECT(count(s, "kind=") == 4 && count(s, " strided=1") == 3 && count(s, "pool=1") == 1);
        CHECK(emb_plan_launch(p, nullptr));
        std::vector<Launch> ls = take_launches();
        EXPECT(ls.size() == 4);
        size_t strided = 0, descs = 0;
        for (const Launch &l : ls) {
            const bool tw = has(l.kernel, "bag_strided_");
            strided += tw;
            descs += l.stride_word.size();
            for (uint64_t v : l.stride_word) EXPECT(v == (tw ? W : 0));
            if (tw) EXPECT(!has(l.kernel, "bag_sum_") && !has(l.kernel, "bag_pool_"));
            if (has(l.kernel, "bag_strided_pool_")) EXPECT(l.stride_word.size() == 1);
        }
        EXPECT(strided == 3 && descs == 5);
        CHECK(emb_plan_destroy(p));
        // the same as a plan-less call, unchecked, checked and deferred
        for (uint32_t check = 0; check < 3; check++) {
            uint64_t bad = 9;
            CHECK(emb_lookup_strided(e, d, ps, st, 5, EMB_IDX_U32, nullptr, check, &bad));
            EXPECT(bad == 0);
            size_t n = 0;
            for (const Launch &l : take_launches())
                if (has(l.kernel, "bag_strided_")) {
                    n++;
                    for (uint64_t v : l.stride_word) EXPECT(v == W);
                } else
                    for (uint64_t v : l.stride_word) EXPECT(v == 0);
            EXPECT(n == 3);
        }
        CHECK(emb_check_report(e, nullptr));
    }

    // ---- plan text, signature, bytes ------------------------------------------------------------------------------------------
    {
        emb_lookup_desc d[2] = {desc(0, buf + 4), desc(0, buf + 4 + D)};
        uint64_t st[2] = {W, W}, dense0[2] = {0, 0}, dense_dim[2] = {D, 0};
        emb_plan *a, *b, *c, *s, *n;
        uint64_t sa, sb, sc, ss, sn, ba, bs;
        char ta[2048], tb[2048], tc[2048], ts[2048];
        CHECK(emb_plan_create_pooled(e, d, nullptr, 2, EMB_IDX_U32, &a));
        CHECK(emb_plan_create_strided(e, d, nullptr, dense0, 2, EMB_IDX_U32, &b));
        CHECK(emb_plan_create_strided(e, d, nullptr, dense_dim, 2, EMB_IDX_U32, &c));
        CHECK(emb_plan_create_strided(e, d, nullptr, st, 2, EMB_IDX_U32, &s));
        CHECK(emb_plan_create_strided(e, d, nullptr, nullptr, 2, EMB_IDX_U32, &n));
        CHECK(emb_plan_signature(a, &sa)); CHECK(emb_plan_signature(b, &sb)); CHECK(emb_plan_signature(c, &sc));
        CHECK(emb_plan_signature(s, &ss)); CHECK(emb_plan_signature(n, &sn));
        EXPECT(sa == sb && sa == sc && sa == sn && sa != ss);
        CHECK(emb_plan_describe(a, ta, sizeof ta)); CHECK(emb_plan_describe(b, tb, sizeof tb)); CHECK(emb_plan_describe(c, tc, sizeof tc));
        CHECK(emb_plan_describe(s, ts, sizeof ts));
        printf("dense:   %s\nstrided: %s\n", ta, ts);
        EXPECT(!strcmp(ta, tb) && !strcmp(ta, tc) && strstr(ta, "strided") == nullptr);
        EXPECT(std::string(ts) == std::string(ta) + " strided=1");
        CHECK(emb_plan_bytes(a, &ba, nullptr, nullptr)); CHECK(emb_plan_bytes(s, &bs, nullptr, nullptr));
        EXPECT(ba == bs);                                                  // the same bytes move
        uint64_t other[2] = {W + 4, W + 4}; emb_plan *o; uint64_t so;
        CHECK(emb_plan_create_strided(e, d, nullptr, other, 2, EMB_IDX_U32, &o));
        CHECK(emb_plan_signature(o, &so));
        EXPECT(so != ss);                                                  // another layout, another plan
        (void)take_launches();
        CHECK(emb_plan_launch(b, nullptr)); CHECK(emb_plan_launch(c, nullptr));
        for (const Launch &l : take_launches()) {
            EXPECT(has(l.kernel, "bag_sum_") && l.stride_word.size() == 2);
            for (uint64_t v : l.stride_word) EXPECT(v == 0);
        }
        for (emb_plan *q : {a, b, c, s, n, o}) CHECK(emb_plan_destroy(q));
    }

    // ---- every other launch keeps the word zero: the batched call, a ranged launch, a queue flush ---------------------------
    {
        emb_lookup_desc d = desc(0, static_cast<float *>(down));
        CHECK(emb_lookup_batched(e, &d, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr));
        emb_lookup_desc r{0, 1, di, nullptr, B, B, static_cast<float *>(down)};
        uint64_t row_lo = 0;
        CHECK(emb_lookup_ranged(e, &r, &row_lo, 1, nullptr));
        emb_queue *q = nullptr;
        CHECK(emb_queue_create(e, EMB_IDX_U32, EMB_MEM_DEVICE, &q));
        emb_lookup_desc qd{0, 1, di, nullptr, 8, 8, static_cast<float *>(down)};
        uint64_t ticket = 0;
        CHECK(emb_queue_add(q, &qd, 1, &ticket)); CHECK(emb_queue_add(q, &qd, 1, &ticket));
        uint32_t got = 0;
        CHECK(emb_queue_flush(q, nullptr, &got));
        EXPECT(got == 2);
        CHECK(emb_queue_destroy(q));
        std::vector<Launch> ls = take_launches();
        EXPECT(ls.size() == 3);
        size_t seen = 0;
        for (const Launch &l : ls) {
            EXPECT(!has(l.kernel, "strided"));
            for (uint64_t v : l.stride_word) { EXPECT(v == 0); seen++; }
        }
        EXPECT(seen == 4);
    }

    // ---- a deferred finding is reported once ---------------------------------------------------------------------------------
    {
        emb_lookup_desc d[2] = {desc(0, buf + 4), desc(1, buf + 4 + D)};
        uint64_t st[2] = {W, W}, bad = 0;
        const uint32_t wild = R + 5;
        CHECK(emb_copy_to_device(e, static_cast<char *>(di) + 20, &wild, 4));
        EXPECT(emb_lookup_strided(e, d, nullptr, st, 2, EMB_IDX_U32, nullptr, 1, &bad) == EMB_ERR_RANGE && bad == 2);   // (both descriptors read it)
        CHECK(emb_lookup_strided(e, d, nullptr, st, 2, EMB_IDX_U32, nullptr, 2, nullptr));      // deferred: not waited for
        CHECK(emb_copy_to_device(e, static_cast<char *>(di) + 20, &idx[5], 4));
        EXPECT(emb_check_report(e, &bad) == EMB_ERR_RANGE && bad == 2);
        CHECK(emb_check_report(e, &bad));
        EXPECT(bad == 0);
        CHECK(emb_lookup_strided(e, d, nullptr, st, 2, EMB_IDX_U32, nullptr, 2, nullptr));
        CHECK(emb_check_report(e, &bad));
    }
    emb_stats stt; CHECK(emb_get_stats(e, &stt));
    printf("launches by kind: %llu %llu %llu %llu %llu\n", (unsigned long long)stt.n_launches_by_kind[0], (unsigned long long)stt.n_launches_by_kind[1],
           (unsigned long long)stt.n_launches_by_kind[2], (unsigned long long)stt.n_launches_by_kind[3], (unsigned long long)stt.n_launches_by_kind[4]);
    for (void *q : {di, dof, dw, dbuf, down}) CHECK(emb_device_free(e, q));
    CHECK(emb_destroy(e));
    printf("strided-out host logic ok\n");
    return 0;
}
