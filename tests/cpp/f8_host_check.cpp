// f8_host_check -- the HOST side of the fp8 table dtypes (EMB_F8_E4M3 / EMB_F8_E5M2, pimemb.h) against
// tests/cpp/hip_runtime_stub.cpp, for AddressSanitizer + UBSan: kernels are no-ops there and "device" memory is host memory, so
// what is checked is what the engine does around the launch.  Tables loaded from EXACTLY sized 1-byte buffers (a staging copy that
// still counted 2 or 4 bytes per element reads past them), HOST calls with check 0 / 1 / 2, hot-row staging, plans (bytes at one
// byte per gathered element, dtype=8 / dtype=9 in the text, a signature of their own), the refusals, the request queue and a
// one-rank shard over every placement.  Linked with the library's host objects as tests/cpp/build_host_logic_check.sh builds
// them (tests/test_f8_cpu.py); nothing of this is linked into libpimemb.so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>
#include "pimemb.h"
#define CHECK(x) do { int rc_ = (x); if (rc_ != EMB_OK) { printf("FAIL %s:%d rc=%d %s\n", __FILE__, __LINE__, rc_, emb_last_error()); exit(1);} } while (0)
#define EXPECT(c) do { if (!(c)) { printf("EXPECT failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, emb_last_error()); exit(1);} } while (0)
// (the sharded call's RCCL binding is not linked: the one-rank shard below has no communicator)
extern "C" int emb_comm_rank(const emb_comm *, int32_t *, int32_t *) { return EMB_ERR_UNSUPPORTED; }
extern "C" int emb_comm_exchange(emb_comm *, const emb_comm_op *, uint32_t, void *) { return EMB_ERR_UNSUPPORTED; }

int main() {
    emb_config cfg{}; cfg.device = 0; cfg.max_tables = 16;
    emb_engine *e = nullptr; CHECK(emb_create(&cfg, &e));
    const uint32_t R = 100;
    // (the two values are passed as the header spells them, never read back out of an emb_dtype object: they lie outside the
    // enum's range, and C++ -- and -fsanitize=enum -- has no defined read of such an object)
    // exactly sized 1-byte tables: dim 16 (one lane per row), 64, 10 (any-dim, element), 36 (any-dim, piece)
    const uint32_t dims[4] = {16, 64, 10, 36};
    std::vector<std::vector<uint8_t>> rows;
    for (uint32_t k = 0; k < 2; k++)
        for (uint32_t j = 0; j < 4; j++) {
            rows.emplace_back((size_t)R * dims[j], (uint8_t)0x38);
            if (k == 0) CHECK(emb_load_table(e, k * 4 + j, R, dims[j], EMB_F8_E4M3, rows.back().data(), EMB_MEM_HOST));
            else CHECK(emb_load_table(e, k * 4 + j, R, dims[j], EMB_F8_E5M2, rows.back().data(), EMB_MEM_HOST));
        }
    std::vector<uint16_t> h16(R * 16, 0x3c00);
    CHECK(emb_load_table(e, 8, R, 16, EMB_BF16, h16.data(), EMB_MEM_HOST));
    // table info, resident bytes
    for (uint32_t k = 0; k < 2; k++) {
        uint64_t n = 0; uint32_t d = 0; emb_dtype dt = EMB_F32; void *p = nullptr;
        CHECK(emb_table_info(e, k * 4 + 1, &p, &n, &d, &dt));
        int dtv = -1; memcpy(&dtv, &dt, sizeof dtv);
        EXPECT(n == R && d == 64 && dtv == 8 + (int)k && p != nullptr);
    }
    emb_stats st; CHECK(emb_get_stats(e, &st));
    EXPECT(st.table_bytes == 2ull * R * (16 + 64 + 10 + 36) + (uint64_t)R * 16 * 2);
    CHECK(emb_alloc_table(e, 9, R, 128, EMB_F8_E4M3));
    CHECK(emb_get_stats(e, &st));
    EXPECT(st.table_bytes == 2ull * R * (16 + 64 + 10 + 36) + (uint64_t)R * 16 * 2 + (uint64_t)R * 128);
    // values 4-7 stay invalid, and so does anything beyond 9
    EXPECT(emb_alloc_table(e, 10, R, 16, (emb_dtype)4) == EMB_ERR_INVALID && emb_alloc_table(e, 10, R, 16, (emb_dtype)5) == EMB_ERR_INVALID);
    EXPECT(emb_alloc_table(e, 10, R, 16, (emb_dtype)6) == EMB_ERR_INVALID && emb_alloc_table(e, 10, R, 16, (emb_dtype)7) == EMB_ERR_INVALID);
    EXPECT(emb_alloc_table(e, 10, R, 16, (emb_dtype)10) == EMB_ERR_INVALID && emb_alloc_table(e, 10, R, 16, (emb_dtype)24) == EMB_ERR_INVALID);

    const uint32_t B = 37;
    std::vector<uint32_t> idx(B * 3), off(B);
    for (uint32_t b = 0; b < B; b++) off[b] = 3 * b;
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (uint32_t)(i * 7 % R);
    std::vector<float> w(idx.size(), 1.f);
    // HOST calls, every table of both dtypes in one call, exactly sized fp32 outputs
    std::vector<std::vector<float>> outs;
    std::vector<emb_lookup_desc> d;
    for (uint32_t t = 0; t < 8; t++) {
        outs.emplace_back((size_t)B * dims[t % 4], 1.f);
        d.push_back(emb_lookup_desc{t, 0, idx.data(), off.data(), idx.size(), B, outs.back().data()});
    }
    CHECK(emb_lookup_batched(e, d.data(), 8, EMB_IDX_U32, EMB_MEM_HOST, nullptr));
    std::vector<emb_pool_spec> ps(8);
    for (uint32_t t = 0; t < 8; t++) ps[t] = emb_pool_spec{t % 3 == 0 ? EMB_POOL_MEAN : t % 3 == 1 ? EMB_POOL_MAX : EMB_POOL_SUM, t % 2 ? EMB_POOL_PADDING : 0u, t % 3 == 2 ? w.data() : nullptr, 3};
    for (uint32_t check = 0; check < 3; check++) {
        uint64_t bad = 0;
        CHECK(emb_lookup_pooled(e, d.data(), ps.data(), 8, EMB_IDX_U32, EMB_MEM_HOST, nullptr, check, &bad));
    }
    // hot rows: 1-byte rows are staged (set and learned)
    const uint64_t hot[5] = {0, 7, 14, 21, 99};
    CHECK(emb_set_hot_rows(e, 1, hot, 5));
    CHECK(emb_set_hot_rows(e, 5, hot, 5));
    uint32_t n_hot = 0; float share = 0.f;
    CHECK(emb_learn_hot_rows(e, 0, idx.data(), idx.size(), EMB_IDX_U32, EMB_MEM_HOST, 8, 0.01f, nullptr, &n_hot, &share));
    EXPECT(n_hot > 0 && n_hot <= 8);
    CHECK(emb_lookup_batched(e, d.data(), 8, EMB_IDX_U32, EMB_MEM_HOST, nullptr));

    // device buffers + plans
    void *di, *dof;
    CHECK(emb_device_alloc(e, idx.size() * 4, &di)); CHECK(emb_device_alloc(e, B * 4, &dof));
    CHECK(emb_copy_to_device(e, di, idx.data(), idx.size() * 4)); CHECK(emb_copy_to_device(e, dof, off.data(), B * 4));
    void *dout[9];
    for (uint32_t t = 0; t < 8; t++) CHECK(emb_device_alloc(e, (size_t)B * dims[t % 4] * 4, &dout[t]));
    CHECK(emb_device_alloc(e, (size_t)B * 16 * 4, &dout[8]));
    uint64_t sig[3] = {0, 0, 0};
    for (uint32_t k = 0; k < 3; k++) {          // e4m3, e5m2, bf16 at dim 16: the same shape, three signatures, two byte counts
        const uint32_t t = k < 2 ? k * 4 : 8;
        emb_lookup_desc dd{t, 0, di, dof, idx.size(), B, (float *)dout[t]};
        emb_plan *p = nullptr; char buf[2048]; uint64_t bytes = 0, nb = 0, ni = 0;
        CHECK(emb_plan_create(e, &dd, 1, EMB_IDX_U32, &p));
        CHECK(emb_plan_describe(p, buf, sizeof buf)); printf("plan %u: %s\n", k, buf);
        CHECK(emb_plan_bytes(p, &bytes, &nb, &ni)); CHECK(emb_plan_signature(p, &sig[k]));
        const uint64_t esz = k < 2 ? 1 : 2;
        EXPECT(nb == B && ni == idx.size());
        EXPECT(bytes == ni * (16 * esz + 4) + (uint64_t)B * 4 + (uint64_t)B * 16 * 4);
        char want[32]; snprintf(want, sizeof want, " dtype=%d ", k < 2 ? 8 + (int)k : 3);
        EXPECT(strstr(buf, want) != nullptr && strstr(buf, k < 2 ? "lanes_per_row=1 chunks=1 " : "lanes_per_row=2 chunks=2 ") != nullptr && strstr(buf, "out=") == nullptr);
        EXPECT(strstr(buf, k == 0 ? "kind=4 " : "kind=1 ") != nullptr);      // (table 0 learned a hot set above: the hot-row launch)
        CHECK(emb_plan_launch(p, nullptr)); CHECK(emb_plan_destroy(p));
    }
    EXPECT(sig[0] != sig[1] && sig[0] != sig[2] && sig[1] != sig[2]);
    {   // any-dim geometry of 1-byte rows: dim 10 by element, dim 36 by 16-byte piece; dim 64 is four lanes per row
        emb_lookup_desc dd[3] = {{2, 0, di, dof, idx.size(), B, (float *)dout[2]}, {3, 0, di, dof, idx.size(), B, (float *)dout[3]}, {1, 0, di, dof, idx.size(), B, (float *)dout[1]}};
        emb_plan *p = nullptr; char buf[4096];
        CHECK(emb_plan_create(e, dd, 3, EMB_IDX_U32, &p));
        CHECK(emb_plan_describe(p, buf, sizeof buf)); printf("shapes: %s\n", buf);
        EXPECT(strstr(buf, "kind=3 dtype=8 itype=0 lanes_per_row=0 chunks=10 scalar_lanes=16 anydim_vec=0") != nullptr);
        EXPECT(strstr(buf, "kind=3 dtype=8 itype=0 lanes_per_row=0 chunks=36 scalar_lanes=4 anydim_vec=1") != nullptr);
        EXPECT(strstr(buf, "dtype=8 itype=0 lanes_per_row=4 chunks=4 ") != nullptr);
        CHECK(emb_plan_launch(p, nullptr)); CHECK(emb_plan_destroy(p));
        emb_pool_spec pp[3] = {{EMB_POOL_MEAN, 0, nullptr, 0}, {EMB_POOL_MAX, 0, nullptr, 0}, {EMB_POOL_MEAN, EMB_POOL_PADDING, nullptr, 3}};
        CHECK(emb_plan_create_pooled(e, dd, pp, 3, EMB_IDX_U32, &p));
        CHECK(emb_plan_describe(p, buf, sizeof buf)); printf("pooled: %s\n", buf);
        EXPECT(strstr(buf, "dtype=8") != nullptr && strstr(buf, "pool=") != nullptr);
        CHECK(emb_plan_launch(p, nullptr)); CHECK(emb_plan_destroy(p));
    }
    // ranged, counted, open end
    {
        std::vector<uint32_t> one(B);
        for (uint32_t b = 0; b < B; b++) one[b] = b * 5 % (R + 20);
        void *d1; CHECK(emb_device_alloc(e, B * 4, &d1)); CHECK(emb_copy_to_device(e, d1, one.data(), B * 4));
        void *ctr; CHECK(emb_device_alloc(e, (size_t)EMB_SERVED_LANES * EMB_SERVED_STRIDE, &ctr));
        emb_lookup_desc dd{5, 1, d1, nullptr, B, B, (float *)dout[5]};
        const uint64_t lo = 10 | EMB_RANGE_OPEN_END; uint32_t *served[1] = {(uint32_t *)ctr};
        CHECK(emb_lookup_ranged_typed(e, &dd, &lo, served, 1, EMB_IDX_U32, nullptr));
        emb_plan *p = nullptr; char buf[1024];
        CHECK(emb_plan_create_ranged_typed(e, &dd, &lo, served, 1, EMB_IDX_U32, &p));
        CHECK(emb_plan_describe(p, buf, sizeof buf)); printf("ranged: %s\n", buf);
        EXPECT(strstr(buf, "dtype=9") != nullptr && strstr(buf, "ranged=1") != nullptr);
        CHECK(emb_plan_destroy(p));
        emb_lookup_desc anyd{2, 1, d1, nullptr, B, B, (float *)dout[2]};
        EXPECT(emb_lookup_ranged_typed(e, &anyd, &lo, nullptr, 1, EMB_IDX_U32, nullptr) == EMB_ERR_UNSUPPORTED);      // dim 10: no lane pieces
        CHECK(emb_synchronize(e, nullptr));
        CHECK(emb_device_free(e, d1)); CHECK(emb_device_free(e, ctr));
    }
    // refusals: no fp8 output, no column loads
    {
        emb_lookup_desc dd{0, 0, di, dof, idx.size(), B, (float *)dout[0]};
        emb_pool_spec hs{EMB_POOL_SUM, EMB_POOL_OUT_TABLE_DTYPE, nullptr, 0}, hm{EMB_POOL_MEAN, EMB_POOL_OUT_TABLE_DTYPE, nullptr, 0};
        emb_plan *p = nullptr;
        EXPECT(emb_lookup_pooled(e, &dd, &hs, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr) == EMB_ERR_UNSUPPORTED);
        EXPECT(emb_lookup_pooled(e, &dd, &hm, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr) == EMB_ERR_UNSUPPORTED);
        dd.table_id = 4;
        EXPECT(emb_plan_create_pooled(e, &dd, &hs, 1, EMB_IDX_U32, &p) == EMB_ERR_UNSUPPORTED);
        std::vector<int32_t> col(R, 1);
        EXPECT(emb_load_table_column(e, 0, 0, col.data(), R) == EMB_ERR_INVALID);
        EXPECT(emb_load_table_column(e, 4, 0, col.data(), R) == EMB_ERR_INVALID);
    }
    // the request queue: one row shape per queue, fp8 as any other
    {
        emb_queue *q = nullptr; CHECK(emb_queue_create(e, EMB_IDX_U32, EMB_MEM_HOST, &q));
        std::vector<std::vector<float>> qo;
        uint64_t tickets[8];
        for (uint32_t r = 0; r < 8; r++) {
            qo.emplace_back((size_t)B * 64, 1.f);
            emb_lookup_desc dd{1, 0, idx.data(), off.data(), idx.size(), B, qo.back().data()};
            CHECK(emb_queue_add(q, &dd, 1, &tickets[r]));
        }
        emb_lookup_desc other{5, 0, idx.data(), off.data(), idx.size(), B, outs[5].data()};      // the same dim, the other encoding
        uint64_t tk = 0;
        EXPECT(emb_queue_add(q, &other, 1, &tk) == EMB_ERR_UNSUPPORTED);
        uint32_t n = 0; CHECK(emb_queue_flush(q, nullptr, &n)); EXPECT(n == 8);
        for (uint32_t r = 0; r < 8; r++) CHECK(emb_queue_wait(q, tickets[r]));
        CHECK(emb_queue_destroy(q));
    }
    // a one-rank shard over every placement (the exchange carries fp32 rows: only the element size of what the rank holds matters)
    for (uint32_t k = 0; k < 2; k++) {
        const uint32_t t64 = k * 4 + 1;
        emb_shard_table tabs[3] = {{EMB_PLACE_REPLICATED, 0, t64, 0}, {EMB_PLACE_WHOLE, 0, t64, 0}, {EMB_PLACE_ROWS, 0, t64, R}};
        for (uint32_t flags : {0u, (uint32_t)EMB_SHARD_CHECK_SERVED, (uint32_t)EMB_SHARD_NO_DIRECT}) {
            emb_shard_config sc{}; sc.n_tables = 3; sc.dim = 64; sc.depth = 0; sc.flags = flags; sc.tables = tabs;
            emb_shard *s = nullptr; CHECK(emb_shard_create(e, nullptr, &sc, &s));
            void *so[3]; emb_shard_input in[3];
            for (int t = 0; t < 3; t++) { CHECK(emb_device_alloc(e, (size_t)B * 64 * 4, &so[t])); in[t] = emb_shard_input{di, dof, idx.size(), 0u, EMB_IDX_U32, (float *)so[t]}; }
            CHECK(emb_shard_lookup(s, in, B, nullptr));
            void *d1; CHECK(emb_device_alloc(e, B * 4, &d1)); CHECK(emb_copy_to_device(e, d1, idx.data(), B * 4));
            for (int t = 0; t < 3; t++) in[t] = emb_shard_input{d1, nullptr, B, 1u, EMB_IDX_U32, (float *)so[t]};      // one index per bag: the direct path
            CHECK(emb_shard_lookup(s, in, B, nullptr));
            emb_shard_stats ss{}; CHECK(emb_shard_get_stats(s, &ss, 0));
            EXPECT(ss.n_batches == 2);
            CHECK(emb_shard_destroy(s));
            CHECK(emb_device_free(e, d1));
            for (int t = 0; t < 3; t++) CHECK(emb_device_free(e, so[t]));
        }
    }
    CHECK(emb_get_stats(e, &st));
    printf("launches by kind: %llu %llu %llu %llu %llu\n", (unsigned long long)st.n_launches_by_kind[0], (unsigned long long)st.n_launches_by_kind[1],
           (unsigned long long)st.n_launches_by_kind[2], (unsigned long long)st.n_launches_by_kind[3], (unsigned long long)st.n_launches_by_kind[4]);
    CHECK(emb_device_free(e, di)); CHECK(emb_device_free(e, dof));
    for (void *q : dout) CHECK(emb_device_free(e, q));
    CHECK(emb_destroy(e));
    printf("f8 host logic ok\n");
    return 0;
}
