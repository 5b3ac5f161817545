// mxfp4_host_check -- the HOST side of MXFP4 tables (EMB_MXFP4, pimemb.h) against tests/cpp/hip_runtime_stub.cpp, for
// AddressSanitizer + UBSan: kernels are no-ops there and "device" memory is host memory, so what is checked is what the engine
// does around the launch.  Tables loaded from EXACTLY sized buffers of fused rows (a copy that counted dim * element bytes, or
// the unpadded row, reads past them or short of them), alloc, info, resident bytes, HOST calls with check 0 / 1 / 2, plans
// (bytes at one row stride per gathered row, dtype=10 and kind=1 in the text whatever the shape), the request queue, every
// refusal and both dim errors.  Linked with the library's host objects as tests/cpp/build_host_logic_check.sh builds them
// (tests/test_mxfp4_cpu.py); nothing of this is linked into libpimemb.so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pimemb.h"
#define CHECK(x) do { int rc_ = (x); if (rc_ != EMB_OK) { printf("FAIL %s:%d rc=%d %s\n", __FILE__, __LINE__, rc_, emb_last_error()); exit(1);} } while (0)
#define EXPECT(c) do { if (!(c)) { printf("EXPECT failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, emb_last_error()); exit(1);} } while (0)
// an EMB_ERR_UNSUPPORTED whose text names the format
#define REFUSED(x) do { int rc_ = (x); if (rc_ != EMB_ERR_UNSUPPORTED || strstr(emb_last_error(), "MXFP4") == nullptr) { \
    printf("not refused as MXFP4 %s:%d: %s -> rc=%d (%s)\n", __FILE__, __LINE__, #x, rc_, emb_last_error()); exit(1);} } while (0)
// (the sharded call's RCCL binding is not linked)
extern "C" int emb_comm_rank(const emb_comm *, int32_t *, int32_t *) { return EMB_ERR_UNSUPPORTED; }
extern "C" int emb_comm_exchange(emb_comm *, const emb_comm_op *, uint32_t, void *) { return EMB_ERR_UNSUPPORTED; }

static_assert(EMB_MXFP4_ROW_BYTES(128u) == 68u && EMB_MXFP4_ROW_STRIDE(32u) == 32u && EMB_MXFP4_ROW_STRIDE(64u) == 48u &&
              EMB_MXFP4_ROW_STRIDE(128u) == 80u && EMB_MXFP4_ROW_STRIDE(256u) == 144u && EMB_MXFP4_ROW_STRIDE(512u) == 272u &&
              EMB_MXFP4_ROW_STRIDE(2048u) == 1088u, "the strides pimemb.h lists");

int main() {
    emb_config cfg{}; cfg.device = 0; cfg.max_tables = 16;
    emb_engine *e = nullptr; CHECK(emb_create(&cfg, &e));
    const uint32_t R = 100;
    // exactly sized tables of fused rows: 1, 2, 3 (of 4), 4, 16 and 64 lanes per row
    const uint32_t dims[6] = {32, 64, 96, 128, 512, 2048};
    std::vector<std::vector<uint8_t>> rows;
    uint64_t resident = 0;
    for (uint32_t j = 0; j < 6; j++) {
        rows.emplace_back((size_t)R * EMB_MXFP4_ROW_STRIDE(dims[j]), (uint8_t)0x22);
        for (uint32_t r = 0; r < R; r++)
            memset(rows.back().data() + (size_t)r * EMB_MXFP4_ROW_STRIDE(dims[j]) + dims[j] / 2, 127, dims[j] / 32);
        CHECK(emb_load_table(e, j, R, dims[j], EMB_MXFP4, rows.back().data(), EMB_MEM_HOST));
        resident += (uint64_t)R * EMB_MXFP4_ROW_STRIDE(dims[j]);
    }
    std::vector<float> h32(R * 32, 1.f);
    CHECK(emb_load_table(e, 6, R, 32, EMB_F32, h32.data(), EMB_MEM_HOST));
    resident += (uint64_t)R * 32 * 4;
    for (uint32_t j = 0; j < 6; j++) {
        uint64_t n = 0; uint32_t d = 0; emb_dtype dt = EMB_F32; void *p = nullptr;
        CHECK(emb_table_info(e, j, &p, &n, &d, &dt));
        int dtv = -1; memcpy(&dtv, &dt, sizeof dtv);
        EXPECT(n == R && d == dims[j] && dtv == 10 && p != nullptr);
        // the rows arrived as they were handed in: a straight copy of R strides
        EXPECT(memcmp(p, rows[j].data(), rows[j].size()) == 0);
    }
    emb_stats st; CHECK(emb_get_stats(e, &st));
    EXPECT(st.table_bytes == resident);
    CHECK(emb_alloc_table(e, 7, R, 256, EMB_MXFP4));
    CHECK(emb_get_stats(e, &st));
    EXPECT(st.table_bytes == resident + (uint64_t)R * 144);
    // both dim errors
    EXPECT(emb_alloc_table(e, 8, R, 48, EMB_MXFP4) == EMB_ERR_INVALID && strstr(emb_last_error(), "MXFP4") != nullptr);
    EXPECT(emb_alloc_table(e, 8, R, 16, EMB_MXFP4) == EMB_ERR_INVALID);
    EXPECT(emb_load_table(e, 8, R, 100, EMB_MXFP4, rows[5].data(), EMB_MEM_HOST) == EMB_ERR_INVALID);
    REFUSED(emb_alloc_table(e, 8, R, 4096, EMB_MXFP4));
    REFUSED(emb_alloc_table(e, 8, R, 2080, EMB_MXFP4));
    EXPECT(emb_alloc_table(e, 8, R, 32, (emb_dtype)11) == EMB_ERR_INVALID);

    const uint32_t B = 37;
    std::vector<uint32_t> idx(B * 3), off(B);
    for (uint32_t b = 0; b < B; b++) off[b] = 3 * b;
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (uint32_t)(i * 7 % R);
    std::vector<float> w(idx.size(), 1.f);
    // HOST calls, every MXFP4 table and the fp32 one in one call, exactly sized fp32 outputs
    std::vector<std::vector<float>> outs;
    std::vector<emb_lookup_desc> d;
    for (uint32_t t = 0; t < 7; t++) {
        outs.emplace_back((size_t)B * (t < 6 ? dims[t] : 32), 1.f);
        d.push_back(emb_lookup_desc{t, 0, idx.data(), off.data(), idx.size(), B, outs.back().data()});
    }
    CHECK(emb_lookup_batched(e, d.data(), 7, EMB_IDX_U32, EMB_MEM_HOST, nullptr));
    CHECK(emb_lookup(e, 3, idx.data(), idx.size(), off.data(), B, outs[3].data(), EMB_IDX_U32, EMB_MEM_HOST, nullptr));
    std::vector<emb_pool_spec> ps(7);
    for (uint32_t t = 0; t < 7; t++) ps[t] = emb_pool_spec{t % 3 == 0 ? EMB_POOL_MEAN : t % 3 == 1 ? EMB_POOL_MAX : EMB_POOL_SUM, t % 2 ? EMB_POOL_PADDING : 0u, t % 3 == 2 ? w.data() : nullptr, 3};
    for (uint32_t check = 0; check < 3; check++) {
        uint64_t bad = 0;
        CHECK(emb_lookup_pooled(e, d.data(), ps.data(), 7, EMB_IDX_U32, EMB_MEM_HOST, nullptr, check, &bad));
    }
    {
        uint64_t bad = 0;
        CHECK(emb_lookup_batched_checked(e, d.data(), 7, EMB_IDX_U32, EMB_MEM_HOST, nullptr, &bad));
    }

    // device buffers + plans
    void *di, *dof;
    CHECK(emb_device_alloc(e, idx.size() * 4, &di)); CHECK(emb_device_alloc(e, B * 4, &dof));
    CHECK(emb_copy_to_device(e, di, idx.data(), idx.size() * 4)); CHECK(emb_copy_to_device(e, dof, off.data(), B * 4));
    void *dout[7];
    for (uint32_t t = 0; t < 7; t++) CHECK(emb_device_alloc(e, (size_t)B * (t < 6 ? dims[t] : 32) * 4, &dout[t]));
    const uint32_t lpr_of[6] = {1, 2, 4, 4, 16, 64};
    uint64_t sig[7];
    for (uint32_t t = 0; t < 7; t++) {
        emb_lookup_desc dd{t, 0, di, dof, idx.size(), B, (float *)dout[t]};
        emb_plan *p = nullptr; char buf[2048], want[96]; uint64_t bytes = 0, nb = 0, ni = 0;
        CHECK(emb_plan_create(e, &dd, 1, EMB_IDX_U32, &p));
        CHECK(emb_plan_describe(p, buf, sizeof buf)); printf("plan %u: %s\n", t, buf);
        CHECK(emb_plan_bytes(p, &bytes, &nb, &ni)); CHECK(emb_plan_signature(p, &sig[t]));
        EXPECT(nb == B && ni == idx.size());
        if (t < 6) {
            EXPECT(bytes == ni * ((uint64_t)EMB_MXFP4_ROW_STRIDE(dims[t]) + 4) + (uint64_t)B * 4 + (uint64_t)B * dims[t] * 4);
            snprintf(want, sizeof want, "kind=1 dtype=10 itype=0 lanes_per_row=%u chunks=%u scalar_lanes=0 anydim_vec=0 ranged=0 ", lpr_of[t], dims[t] / 32);
            EXPECT(strstr(buf, want) != nullptr && strstr(buf, "out=") == nullptr && strstr(buf, "pool=") == nullptr);
        } else {
            EXPECT(bytes == ni * (32ull * 4 + 4) + (uint64_t)B * 4 + (uint64_t)B * 32 * 4);      // (the other dtypes' figures have not moved)
            EXPECT(strstr(buf, " dtype=0 ") != nullptr);
        }
        CHECK(emb_plan_launch(p, nullptr)); CHECK(emb_plan_destroy(p));
    }
    for (uint32_t a = 0; a < 7; a++)
        for (uint32_t b = a + 1; b < 7; b++) EXPECT(sig[a] != sig[b]);
    {   // a big one-hot launch, the shape choose_kernel gives the wave-batch kernels: MXFP4 stays on the lane-group kernel
        const uint32_t BB = 64 * 2048 * 2;
        std::vector<uint32_t> one(BB);
        for (uint32_t b = 0; b < BB; b++) one[b] = b % R;
        void *d1, *o0, *o6;
        CHECK(emb_device_alloc(e, (size_t)BB * 4, &d1)); CHECK(emb_copy_to_device(e, d1, one.data(), (size_t)BB * 4));
        CHECK(emb_device_alloc(e, (size_t)BB * 32 * 4, &o0)); CHECK(emb_device_alloc(e, (size_t)BB * 32 * 4, &o6));
        emb_lookup_desc dd[2] = {{0, 1, d1, nullptr, BB, BB, (float *)o0}, {6, 1, d1, nullptr, BB, BB, (float *)o6}};
        emb_plan *p = nullptr; char buf[2048];
        CHECK(emb_plan_create(e, dd, 2, EMB_IDX_U32, &p));
        CHECK(emb_plan_describe(p, buf, sizeof buf)); printf("one-hot: %s\n", buf);
        EXPECT(strstr(buf, "kind=1 dtype=10 ") != nullptr && strstr(buf, "kind=0 dtype=0 ") != nullptr);
        CHECK(emb_plan_launch(p, nullptr)); CHECK(emb_plan_destroy(p));
        CHECK(emb_lookup_batched(e, dd, 2, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr));
        CHECK(emb_synchronize(e, nullptr));
        CHECK(emb_device_free(e, d1)); CHECK(emb_device_free(e, o0)); CHECK(emb_device_free(e, o6));
    }
    {   // pooled plans: the three modes, weights, padding
        emb_lookup_desc dd[3] = {{0, 0, di, dof, idx.size(), B, (float *)dout[0]}, {3, 0, di, dof, idx.size(), B, (float *)dout[3]}, {5, 0, di, dof, idx.size(), B, (float *)dout[5]}};
        void *dw; CHECK(emb_device_alloc(e, w.size() * 4, &dw)); CHECK(emb_copy_to_device(e, dw, w.data(), w.size() * 4));
        emb_pool_spec pp[3] = {{EMB_POOL_MEAN, 0, nullptr, 0}, {EMB_POOL_MAX, EMB_POOL_PADDING, nullptr, 3}, {EMB_POOL_SUM, 0, (const float *)dw, 0}};
        emb_plan *p = nullptr; char buf[4096];
        CHECK(emb_plan_create_pooled(e, dd, pp, 3, EMB_IDX_U32, &p));
        CHECK(emb_plan_describe(p, buf, sizeof buf)); printf("pooled: %s\n", buf);
        EXPECT(strstr(buf, "kind=1 dtype=10 itype=0 lanes_per_row=1 ") != nullptr && strstr(buf, "kind=1 dtype=10 itype=0 lanes_per_row=4 ") != nullptr &&
               strstr(buf, "kind=1 dtype=10 itype=0 lanes_per_row=64 ") != nullptr && strstr(buf, "pool=") != nullptr && strstr(buf, "kind=0") == nullptr);
        float us = 0.f;
        CHECK(emb_plan_launch(p, nullptr)); CHECK(emb_plan_time(p, nullptr, 1, 2, &us)); CHECK(emb_plan_destroy(p));
        CHECK(emb_lookup_pooled(e, dd, pp, 3, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr));
        CHECK(emb_synchronize(e, nullptr));
        CHECK(emb_device_free(e, dw));
    }
    // refusals, each naming the format
    {
        std::vector<uint32_t> one(B);
        for (uint32_t b = 0; b < B; b++) one[b] = b * 5 % R;
        void *d1; CHECK(emb_device_alloc(e, B * 4, &d1)); CHECK(emb_copy_to_device(e, d1, one.data(), B * 4));
        void *ctr; CHECK(emb_device_alloc(e, (size_t)EMB_SERVED_LANES * EMB_SERVED_STRIDE, &ctr));
        emb_lookup_desc dd{3, 1, d1, nullptr, B, B, (float *)dout[3]};
        const uint64_t lo = 0; uint32_t *served[1] = {(uint32_t *)ctr};
        emb_plan *p = nullptr;
        REFUSED(emb_lookup_ranged(e, &dd, &lo, 1, nullptr));
        REFUSED(emb_lookup_ranged_counted(e, &dd, &lo, served, 1, nullptr));
        REFUSED(emb_lookup_ranged_typed(e, &dd, &lo, served, 1, EMB_IDX_I64, nullptr));
        REFUSED(emb_plan_create_ranged(e, &dd, &lo, 1, &p));
        REFUSED(emb_plan_create_ranged_counted(e, &dd, &lo, served, 1, &p));
        REFUSED(emb_plan_create_ranged_typed(e, &dd, &lo, served, 1, EMB_IDX_U32, &p));
        EXPECT(p == nullptr);
        CHECK(emb_device_free(e, d1)); CHECK(emb_device_free(e, ctr));

        emb_lookup_desc pd{3, 0, di, dof, idx.size(), B, (float *)dout[3]};
        emb_pool_spec hs{EMB_POOL_SUM, EMB_POOL_OUT_TABLE_DTYPE, nullptr, 0}, hm{EMB_POOL_MEAN, EMB_POOL_OUT_TABLE_DTYPE, nullptr, 0};
        REFUSED(emb_lookup_pooled(e, &pd, &hs, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr));
        REFUSED(emb_lookup_pooled(e, &pd, &hm, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr));
        REFUSED(emb_plan_create_pooled(e, &pd, &hs, 1, EMB_IDX_U32, &p));

        const uint64_t hot[3] = {0, 7, 99};
        REFUSED(emb_set_hot_rows(e, 3, hot, 3));
        uint32_t n_hot = 0; float share = 0.f;
        REFUSED(emb_learn_hot_rows(e, 3, idx.data(), idx.size(), EMB_IDX_U32, EMB_MEM_HOST, 8, 0.01f, nullptr, &n_hot, &share));
        std::vector<int32_t> col(R, 1);
        REFUSED(emb_load_table_column(e, 3, 0, col.data(), R));

        // a one-rank shard: refused where this rank holds an MXFP4 table, fine where it holds none of them
        emb_shard_table tabs[2] = {{EMB_PLACE_REPLICATED, 0, 6, 0}, {EMB_PLACE_ROWS, 0, 0, R}};
        for (uint32_t place : {(uint32_t)EMB_PLACE_REPLICATED, (uint32_t)EMB_PLACE_WHOLE, (uint32_t)EMB_PLACE_ROWS}) {
            tabs[1].placement = place;
            emb_shard_config sc{}; sc.n_tables = 2; sc.dim = 32; sc.depth = 0; sc.flags = 0; sc.tables = tabs;
            emb_shard *s = nullptr;
            REFUSED(emb_shard_create(e, nullptr, &sc, &s));
            EXPECT(s == nullptr);
        }
        emb_shard_config sc{}; sc.n_tables = 1; sc.dim = 32; sc.depth = 0; sc.flags = 0; sc.tables = tabs;
        emb_shard *s = nullptr; CHECK(emb_shard_create(e, nullptr, &sc, &s)); CHECK(emb_shard_destroy(s));
    }
    // the request queue: its fused launch is the lane-group kernel's, so MXFP4 as any other dtype -- one row shape per queue
    {
        emb_queue *q = nullptr; CHECK(emb_queue_create(e, EMB_IDX_U32, EMB_MEM_HOST, &q));
        std::vector<std::vector<float>> qo;
        uint64_t tickets[8];
        for (uint32_t r = 0; r < 8; r++) {
            qo.emplace_back((size_t)B * 128, 1.f);
            emb_lookup_desc dd{3, 0, idx.data(), off.data(), idx.size(), B, qo.back().data()};
            CHECK(emb_queue_add(q, &dd, 1, &tickets[r]));
        }
        emb_lookup_desc other{0, 0, idx.data(), off.data(), idx.size(), B, outs[0].data()};
        uint64_t tk = 0;
        EXPECT(emb_queue_add(q, &other, 1, &tk) == EMB_ERR_UNSUPPORTED);
        uint32_t n = 0; CHECK(emb_queue_flush(q, nullptr, &n)); EXPECT(n == 8);
        for (uint32_t r = 0; r < 8; r++) CHECK(emb_queue_wait(q, tickets[r]));
        CHECK(emb_queue_destroy(q));
    }
    CHECK(emb_get_stats(e, &st));
    printf("launches by kind: %llu %llu %llu %llu %llu\n", (unsigned long long)st.n_launches_by_kind[0], (unsigned long long)st.n_launches_by_kind[1],
           (unsigned long long)st.n_launches_by_kind[2], (unsigned long long)st.n_launches_by_kind[3], (unsigned long long)st.n_launches_by_kind[4]);
    CHECK(emb_device_free(e, di)); CHECK(emb_device_free(e, dof));
    for (void *q : dout) CHECK(emb_device_free(e, q));
    CHECK(emb_destroy(e));
    printf("mxfp4 host logic ok\n");
    return 0;
}
