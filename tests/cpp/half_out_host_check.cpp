// half_out_host_check -- the HOST side of EMB_POOL_OUT_TABLE_DTYPE (pimemb.h) against tests/cpp/hip_runtime_stub.cpp, for
// AddressSanitizer + UBSan: kernels are no-ops there and "device" memory is host memory, so what is checked is what the engine
// does around the launch.  HOST and DEVICE calls with check 0 / 1 / 2 into EXACTLY sized 2-byte outputs (a staging or copy-out
// that still counted 4 bytes per element overruns them), flagged and unflagged descriptors in one call, plans (out=1 in the
// text of flagged launches only, signatures, algorithmic bytes) and the refusals.  Linked with the library's host objects as
// tests/cpp/build_host_logic_check.sh builds them (tests/test_half_out_cpu.py); nothing of this is linked into libpimemb.so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <initializer_list>
#include <vector>
#include "pimemb.h"
#define CHECK(x) do { int rc_ = (x); if (rc_ != EMB_OK) { printf("FAIL %s:%d rc=%d %s\n", __FILE__, __LINE__, rc_, emb_last_error()); exit(1);} } while (0)
#define EXPECT(c) do { if (!(c)) { printf("EXPECT failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, emb_last_error()); exit(1);} } while (0)
// (the sharded call's RCCL binding is not linked: nothing here makes a shard)
extern "C" int emb_comm_rank(const emb_comm *, int32_t *, int32_t *) { return EMB_ERR_UNSUPPORTED; }
extern "C" int emb_comm_exchange(emb_comm *, const emb_comm_op *, uint32_t, void *) { return EMB_ERR_UNSUPPORTED; }

int main() {
    emb_config cfg{}; cfg.device = 0; cfg.max_tables = 8;
    emb_engine *e = nullptr; CHECK(emb_create(&cfg, &e));
    const uint32_t R = 100;
    std::vector<float> f32(R * 16, 0.5f); std::vector<uint16_t> h16(R * 16, 0x3c00), h5(R * 5, 0x3f80); std::vector<int32_t> fx(R * 16, 7);
    CHECK(emb_load_table(e, 0, R, 16, EMB_F32, f32.data(), EMB_MEM_HOST));
    CHECK(emb_load_table(e, 1, R, 16, EMB_F16, h16.data(), EMB_MEM_HOST));
    CHECK(emb_load_table(e, 2, R, 16, EMB_BF16, h16.data(), EMB_MEM_HOST));
    CHECK(emb_load_table(e, 3, R, 16, EMB_FIXED32, fx.data(), EMB_MEM_HOST));
    CHECK(emb_load_table(e, 4, R, 5, EMB_BF16, h5.data(), EMB_MEM_HOST));
    const uint32_t B = 37;
    std::vector<uint32_t> idx(B * 3), off(B);
    for (uint32_t b = 0; b < B; b++) off[b] = 3 * b;
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (uint32_t)(i * 7 % R);
    std::vector<float> w(idx.size(), 1.f);
    // exactly sized outputs: ASan sees a 4-byte-per-element copy into a half buffer
    std::vector<uint16_t> o1(B * 16, 0xAAAA), o2(B * 16, 0xAAAA), o4(B * 5, 0xAAAA);
    std::vector<float> of(B * 16, 0.f);
    emb_lookup_desc d[4] = {{1, 0, idx.data(), off.data(), idx.size(), B, (float *)o1.data()}, {2, 0, idx.data(), off.data(), idx.size(), B, (float *)o2.data()},
                            {4, 0, idx.data(), off.data(), idx.size(), B, (float *)o4.data()}, {1, 0, idx.data(), off.data(), idx.size(), B, of.data()}};
    emb_pool_spec ps[4] = {{EMB_POOL_SUM, EMB_POOL_OUT_TABLE_DTYPE, nullptr, 0}, {EMB_POOL_MEAN, EMB_POOL_OUT_TABLE_DTYPE | EMB_POOL_PADDING, nullptr, 3},
                           {EMB_POOL_SUM, EMB_POOL_OUT_TABLE_DTYPE, w.data(), 0}, {EMB_POOL_SUM, 0, nullptr, 0}};
    for (uint32_t check = 0; check < 3; check++) {
        uint64_t bad = 0;
        CHECK(emb_lookup_pooled(e, d, ps, 4, EMB_IDX_U32, EMB_MEM_HOST, nullptr, check, &bad));
    }
    // device buffers + plans
    void *di, *dof, *dw, *dout[4];
    CHECK(emb_device_alloc(e, idx.size() * 4, &di)); CHECK(emb_device_alloc(e, B * 4, &dof)); CHECK(emb_device_alloc(e, idx.size() * 4, &dw));
    CHECK(emb_copy_to_device(e, di, idx.data(), idx.size() * 4)); CHECK(emb_copy_to_device(e, dof, off.data(), B * 4));
    CHECK(emb_copy_to_device(e, dw, w.data(), idx.size() * 4));
    size_t sz[4] = {B * 16 * 2, B * 16 * 2, B * 5 * 2, B * 16 * 4};
    emb_lookup_desc dd[4]; emb_pool_spec dps[4];
    for (int i = 0; i < 4; i++) { CHECK(emb_device_alloc(e, sz[i], &dout[i])); dd[i] = d[i]; dd[i].indices = di; dd[i].offsets = dof; dd[i].pooled = (float *)dout[i]; dps[i] = ps[i]; }
    dps[2].per_sample_weights = (const float *)dw;
    for (uint32_t check = 0; check < 3; check++) CHECK(emb_lookup_pooled(e, dd, dps, 4, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, check, nullptr));
    CHECK(emb_check_report(e, nullptr));
    emb_plan *p = nullptr; char buf[4096];
    CHECK(emb_plan_create_pooled(e, dd, dps, 4, EMB_IDX_U32, &p));
    CHECK(emb_plan_describe(p, buf, sizeof buf)); printf("mixed: %s\n", buf);
    { std::string s(buf); size_t n = 0, at = 0; while ((at = s.find(" out=1", at)) != std::string::npos) { n++; at++; } EXPECT(n == 3); }
    CHECK(emb_plan_launch(p, nullptr)); CHECK(emb_plan_destroy(p));
    // unflagged: the same plan as emb_plan_create; flagged plain sum: differs, 2 bytes per output element, text = old text + " out=1"
    emb_plan *a, *b, *c; uint64_t sa, sb, sc, ba, bc;
    CHECK(emb_plan_create(e, dd, 2, EMB_IDX_U32, &a));
    emb_pool_spec plain[2] = {{EMB_POOL_SUM, 0, nullptr, 0}, {EMB_POOL_SUM, 0, nullptr, 0}}, half[2] = {ps[0], ps[0]};
    CHECK(emb_plan_create_pooled(e, dd, plain, 2, EMB_IDX_U32, &b)); CHECK(emb_plan_create_pooled(e, dd, half, 2, EMB_IDX_U32, &c));
    CHECK(emb_plan_signature(a, &sa)); CHECK(emb_plan_signature(b, &sb)); CHECK(emb_plan_signature(c, &sc));
    EXPECT(sa == sb && sa != sc);
    CHECK(emb_plan_bytes(a, &ba, nullptr, nullptr)); CHECK(emb_plan_bytes(c, &bc, nullptr, nullptr));
    EXPECT(ba - bc == 2ull * B * 16 * 2);
    char ta[4096], tc[4096]; CHECK(emb_plan_describe(a, ta, sizeof ta)); CHECK(emb_plan_describe(c, tc, sizeof tc));
    printf("plain: %s\nhalf:  %s\n", ta, tc);
    EXPECT(strstr(ta, "out=") == nullptr);
    CHECK(emb_plan_destroy(a)); CHECK(emb_plan_destroy(b)); CHECK(emb_plan_destroy(c));
    // refusals
    emb_lookup_desc r0 = dd[3]; r0.table_id = 0; emb_lookup_desc r3 = dd[3]; r3.table_id = 3;
    emb_pool_spec hs = ps[0], hm = {EMB_POOL_MEAN, EMB_POOL_OUT_TABLE_DTYPE, nullptr, 0}, b4 = {EMB_POOL_SUM, 4, nullptr, 0}, b6 = {EMB_POOL_SUM, 6, nullptr, 0};
    EXPECT(emb_lookup_pooled(e, &r0, &hs, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr) == EMB_ERR_UNSUPPORTED);
    EXPECT(emb_lookup_pooled(e, &r0, &hm, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr) == EMB_ERR_UNSUPPORTED);
    EXPECT(emb_lookup_pooled(e, &r3, &hs, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr) == EMB_ERR_UNSUPPORTED);
    EXPECT(emb_lookup_pooled(e, &r3, &hs, 1, EMB_IDX_U32, EMB_MEM_HOST, nullptr, 1, nullptr) == EMB_ERR_UNSUPPORTED);
    EXPECT(emb_lookup_pooled(e, &dd[0], &b4, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr) == EMB_ERR_INVALID);
    EXPECT(emb_lookup_pooled(e, &dd[0], &b6, 1, EMB_IDX_U32, EMB_MEM_DEVICE, nullptr, 0, nullptr) == EMB_ERR_INVALID);
    EXPECT(emb_plan_create_pooled(e, &r0, &hs, 1, EMB_IDX_U32, &p) == EMB_ERR_UNSUPPORTED);
    emb_stats st; CHECK(emb_get_stats(e, &st));
    printf("launches by kind: %llu %llu %llu %llu %llu\n", (unsigned long long)st.n_launches_by_kind[0], (unsigned long long)st.n_launches_by_kind[1],
           (unsigned long long)st.n_launches_by_kind[2], (unsigned long long)st.n_launches_by_kind[3], (unsigned long long)st.n_launches_by_kind[4]);
    for (void *q : {di, dof, dw, dout[0], dout[1], dout[2], dout[3]}) CHECK(emb_device_free(e, q));
    CHECK(emb_destroy(e));
    printf("half-out host logic ok\n");
    return 0;
}
