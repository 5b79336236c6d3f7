// The context: allocation and environment knobs, stream skew, profiling scopes, read-back, the
// per-call uploads through the pinned staging buffers, the fp64 factors of wide slots.
#include <cmath>
#include <cstdlib>

#include "apm_host.h"

// ------------------------------------------------------------------------------- APM_SKEW
// (tests only) the calling thread's context selects delay kernels in front of every launch on
// its secondary streams (bit 0: chol(K), the posterior's bottom block, the Newton far updates)
// and/or its main stream (bit 1). Every cross-stream edge is an event (Edges); with one side of
// an edge held back by the delays, a missing or misplaced wait shows as a changed result, which
// tests/test_gpu_errors.py::test_stream_skew_is_bitwise_neutral compares bitwise.
namespace {
thread_local apm_host::SkewState t_skew;
constexpr int SKEW_US_SECONDARY = 1000, SKEW_US_MAIN = 40;
}  // namespace

void skew_point(hipStream_t s) {
    if (!t_skew.mode || !s) return;
    if ((t_skew.mode & 1) && (s == t_skew.s2 || s == t_skew.s3))
        launch_delay(SKEW_US_SECONDARY, s);
    else if ((t_skew.mode & 2) && s == t_skew.main)
        launch_delay(SKEW_US_MAIN, s);
}

namespace apm_host {

SkewScope::SkewScope(const apm_ctx* c) : prev(t_skew) {
    t_skew = SkewState{c->skew & 3, c->stream, c->stream2, c->stream3};
}
SkewScope::~SkewScope() { t_skew = prev; }

// ------------------------------------------------------------------------------- profiling
hipEvent_t next_event(apm_ctx* c) {
    if (c->evnext == c->evpool.size()) {
        hipEvent_t e;
        HIPC(hipEventCreate(&e));
        c->evpool.push_back(e);
    }
    return c->evpool[c->evnext++];
}

// ------------------------------------------------------------------------------- transfers
void read_back(apm_ctx* c, std::initializer_list<RB> l) {
    Export e{};
    int k = 0;
    for (const RB& r : l) {
        e.src[k] = static_cast<const unsigned*>(r.src);
        e.words[k] = r.bytes / 4;
        ++k;
    }
    e.dst = c->dx;
    launch_export(e, c->stream);
    sync(c);
    int off = 0;
    for (const RB& r : l) {
        std::memcpy(r.host, reinterpret_cast<const char*>(c->hx) + off, r.bytes);
        off += r.bytes;
    }
}

// slots / ubufs of a call -> device in one copy from pinned memory
void upload_idx(apm_ctx* c, int count, const int64_t* slots, const int64_t* ubufs) {
    int64_t* h = pin_slots(c);
    if (slots) std::memcpy(h, slots, sizeof(int64_t) * count);
    if (ubufs) std::memcpy(pin_ubufs(c), ubufs, sizeof(int64_t) * count);
    if (ubufs)  // [slots | ubufs .. + count) -> d_slots | d_ubufs
        HIPC(hipMemcpyAsync(c->d_slots, h, sizeof(int64_t) * (pin_ubufs(c) + count - h),
                            hipMemcpyHostToDevice, c->stream));
    else if (slots)
        HIPC(hipMemcpyAsync(c->d_slots, h, sizeof(int64_t) * count, hipMemcpyHostToDevice,
                            c->stream));
}

// per-chain range flags of a theta-call (staged by the entry point in pin_h3 / pin_h3post /
// pin_inv, the layout of the device block h3ok .. h3ok + 3B, uploaded with one copy, and the icm
// thresholds in pin_icm) -> device. fp16x3 operands (chol32_update.hip): the walk's and
// the trailing updates' operands are solved entries of L, |L_ij| <= sqrt(B_ii) <= sqrt(1 + K_ii)
// (probit W < 1, logit W <= 1/4); the explicit-inverse panel also splits Schur-complement
// entries of B itself, |A_ij| <= max B_ii <= 1 + K_ii, so its flag asks 1 + K_ii < 2^15 (fp16
// overflows at 65504).
// h3_now = any chain flagged (else the fp32-operand kernels launch), inv_any / inv_all likewise.
void upload_h3(apm_ctx* c, int count) {
    int* h = pin_h3(c);
    int* v = pin_inv(c);
    c->h3_now = c->inv_any = false;
    c->h3_all = c->inv_all = c->h3post_all = count > 0;
    for (int b = 0; b < count; ++b) {
        c->h3post_all &= pin_h3post(c)[b] != 0;
        v[b] = v[b] && h[b];
        c->h3_now |= h[b] != 0;
        c->h3_all &= h[b] != 0;
        c->inv_any |= v[b] != 0;
        c->inv_all &= v[b] != 0;
    }
    // [h3ok | h3post | invok .. + count) -> the device block of the same layout
    HIPC(hipMemcpyAsync(c->h3ok, h, sizeof(int) * (v + count - h), hipMemcpyHostToDevice,
                        c->stream));
    double* t = pin_icm(c);
    for (int b = 0; b < count; ++b) t[b] = c->icm_q > 0.0 ? t[b] : -1.0;
    HIPC(hipMemcpyAsync(c->icm_thr, t, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
}

const double* upload_thetas(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt) {
    double* th = c->hth;  // pinned: the upload is asynchronous
    for (int64_t b = 0; b < count; ++b)
        for (int p = 0; p < c->P; ++p) th[b * c->P + p] = thetas[b * ldt + p];
    HIPC(hipMemcpyAsync(c->theta, th, sizeof(double) * count * c->P, hipMemcpyHostToDevice,
                        c->stream));
    return th;
}

double upload_padded_K(apm_ctx* c, const double* K, int64_t ldk, std::vector<double>& Kp) {
    const int np = c->np;
    Kp = std::vector<double>((size_t)np * np, 0.0);
    for (int i = 0; i < np; ++i)
        for (int j = 0; j < np; ++j)
            Kp[(size_t)i * np + j] =
                (i < c->n && j < c->n) ? K[(int64_t)i * ldk + j] : (i == j ? 1.0 : 0.0);
    HIPC(hipMemcpyAsync(c->K.base, Kp.data(), sizeof(double) * Kp.size(), hipMemcpyHostToDevice,
                        c->stream));
    c->k_full = true;
    double kmax = 0.0;
    for (int i = 0; i < c->n; ++i) kmax = std::max(kmax, std::fabs(Kp[(size_t)i * np + i]));
    return kmax;
}

// fp64 factor buffers of wide slots (Sl.L64): attached on demand, recycled through l64_free
void attach_l64(apm_ctx* c, int64_t slot) {
    if (c->l64_h[slot]) return;
    if (!c->l64_free.empty()) {
        c->l64_h[slot] = c->l64_free.back();
        c->l64_free.pop_back();
    } else {
        c->l64_h[slot] = dalloc<double>(c, c->np * c->np);
    }
}
void detach_l64(apm_ctx* c, int64_t slot) {
    if (!c->l64_h[slot]) return;
    c->l64_free.push_back(c->l64_h[slot]);
    c->l64_h[slot] = nullptr;
}
void upload_l64(apm_ctx* c) {  // pageable source: the copy has read it when the call returns
    HIPC(hipMemcpyAsync(c->l64_d, c->l64_h.data(), sizeof(double*) * c->n_slots,
                        hipMemcpyHostToDevice, c->stream));
}

// ------------------------------------------------------------------------------- the context
void init_ctx(apm_ctx* c, int device, int kind, const double* X, int64_t n, int64_t d,
              int64_t ldx, const double* y, double eps, int64_t S, int64_t max_batch,
              int64_t n_slots, int64_t n_ubufs) {
    c->device = device;
    // the library's environment knobs, read here once per context: two
    // correctness fallbacks (APM_MIXED=0: fp64 Newton factorisation; APM_H3=0: fp32 operands in
    // the fp32 factorisations' outer updates) and test thresholds / test modes that the GPU
    // tests use to reach rare paths. The defaults are the product.
    HIPC(hipSetDevice(device));
    trsv32_mw_init();
    if (const char* e = getenv("APM_MIXED")) c->mixed = atoi(e) != 0;
    if (const char* e = getenv("APM_H3")) c->h3 = atoi(e) != 0;
    // acceptance of a refinement step (test threshold: 0 sends every chain to the fp64 rerun)
    if (const char* e = getenv("APM_REFINE_TOL")) c->refine_tol = atof(e);
    // the reference-route check of chol(C) (icm_check): trace(C) below n K_ii / APM_ICM_Q
    // (test threshold: 1 checks every chain, 0 none)
    if (const char* e = getenv("APM_ICM_Q")) c->icm_q = std::max(0.0, atof(e));
    // poll bound of every in-launch hand-over wait (tests/test_gpu_errors.py forces the
    // bounded-spin exits with 1 and checks that no chain returns a wrong value with status 0)
    if (const char* e = getenv("APM_SPIN_LIMIT")) c->spin_df = c->spin_trsv = std::max(1, atoi(e));
    // delay kernels in front of every launch on the secondary streams (bit 0) and/or on the main
    // stream (bit 1): a cross-stream edge without its wait then gives a wrong result
    // deterministically (tests/test_gpu_errors.py::test_stream_skew_is_bitwise_neutral); bit 2
    // removes one edge's wait (bottom_done) to show that such a result is caught
    if (const char* e = getenv("APM_SKEW")) c->skew = std::max(0, std::min(7, atoi(e)));
    {  // main stream at the highest priority: the concurrent chol(K) only fills idle CUs
        int least = 0, greatest = 0;
        HIPC(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPC(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, greatest));
        HIPC(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, least));
        HIPC(hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, least));
    }
    c->kind = kind;
    c->n = (int)n;
    c->d = (int)d;
    c->np = (int)((n + 63) / 64 * 64);
    c->nb = c->np / 64;
    {  // one event per cross-stream edge (Edges): the per-panel ones indexed by panel
        const int np64 = (c->nb + c->outer - 1) / c->outer, np32 = (c->nb + c->outer32 - 1) / c->outer32;
        c->ev.cholk_rel.assign(np64, nullptr);
        c->ev.lp_panel.assign(np64, nullptr);
        c->ev.df.assign(np32, nullptr);
        c->ev.far.assign(np32, nullptr);
        for (hipEvent_t* e : c->ev.all()) HIPC(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    c->P = (int)kernel_kind_of(kind).theta_len(d);  // (0: APM_KERNEL_PRECOMPUTED)
    c->S = (int)S;
    c->sp = (int)((S + 63) / 64 * 64);
    c->max_batch = (int)max_batch;
    c->n_slots = (int)n_slots;
    c->slot_refs.assign((size_t)n_slots, 0);
    c->n_ubufs = (int)n_ubufs;
    c->eps = eps;
    const int64_t np = c->np, B = max_batch;
    if (kind != APM_KERNEL_PRECOMPUTED && d > 0) {
        c->X = dalloc<double>(c, n * d);
        std::vector<double> Xc((size_t)(n * d));
        for (int64_t i = 0; i < n; ++i)
            for (int64_t k = 0; k < d; ++k) Xc[i * d + k] = X[i * ldx + k];
        HIPC(hipMemcpy(c->X, Xc.data(), sizeof(double) * n * d, hipMemcpyHostToDevice));
        for (int64_t i = 0; i < n; ++i) {  // (the range flags of a kind with the linear term)
            double s = 0.0;
            for (int64_t k = 0; k < d; ++k) s += Xc[i * d + k] * Xc[i * d + k];
            c->x2max = std::max(c->x2max, s);
            c->x2sum += s;
        }
    }
    c->y = dalloc<double>(c, np);
    std::vector<double> yp((size_t)np, 0.0);
    if (y)
        for (int64_t i = 0; i < n; ++i) yp[i] = y[i];
    HIPC(hipMemcpy(c->y, yp.data(), sizeof(double) * np, hipMemcpyHostToDevice));
    c->theta = dalloc<double>(c, B * std::max(c->P, 1));
    c->K = MatB{dalloc<double>(c, B * np * np), np, np * np};
    const int64_t arows = 2 * np + 64, acols = 2 * np;
    c->A = MatB{dalloc<double>(c, B * arows * acols), acols, arows * acols};
    c->dstride = 2 * c->nb * 4096;
    c->Dinv = dalloc<double>(c, B * c->dstride);
    c->lstride = 2 * c->nb;
    c->ldet = dalloc<double>(c, B * c->lstride);
    c->out = dalloc<double>(c, B);
    c->pstride = (int64_t)c->nb * c->sp;
    c->partial = dalloc<double>(c, B * c->pstride);
    const int64_t vs = np;
    c->vecbase = dalloc<double>(c, 8 * B * vs);
    c->rvec = dalloc<double>(c, 3 * B * vs);
    c->sstride = (int64_t)c->nb * c->nb * 64;
    c->sympart = dalloc<double>(c, B * c->sstride);
    c->v = NewtonVecs{c->vecbase,          c->vecbase + 1 * B * vs, c->vecbase + 2 * B * vs,
                      c->vecbase + 3 * B * vs, c->vecbase + 4 * B * vs, c->vecbase + 5 * B * vs,
                      c->vecbase + 6 * B * vs, c->vecbase + 7 * B * vs, vs};
    HIPC(hipMemset(c->vecbase, 0, sizeof(double) * 8 * B * vs));
    c->active = dalloc<int>(c, B);
    c->status = dalloc<int>(c, B);
    c->n_iter = dalloc<int>(c, B);
    c->refining = dalloc<int>(c, B);
    c->active2 = dalloc<int>(c, B);
    c->status2 = dalloc<int>(c, B);
    c->refine_prev = dalloc<double>(c, B);
    c->d_slots = dalloc<int64_t>(c, 2 * B);
    c->d_ubufs = c->d_slots + B;
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&c->hpin), pin_of(c).bytes(),
                       hipHostMallocDefault));
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&c->hmask), sizeof(int) * (size_t)B,
                       hipHostMallocDefault));
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&c->hx), read_back_bytes(B),
                       hipHostMallocMapped | hipHostMallocCoherent));
    HIPC(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->dx), c->hx, 0));
    c->h3ok = dalloc<int>(c, 3 * B);
    c->h3post = c->h3ok + B;
    c->invok = c->h3ok + 2 * B;
    c->guard = dalloc<double>(c, 6 * B);
    HIPC(hipMemset(c->guard, 0, sizeof(double) * 6 * B));
    c->guard_rows = dalloc<double>(c, B * np);
    c->icm_thr = dalloc<double>(c, B);
    if (c->mixed && c->h3) {
        c->plane_cs = 2 * np * 32 * 2 * c->outer32;  // 2 planes x rows x 2 outer32 slices x 32
        // a buffer per outer panel for the left-looking far updates (8 of 537 MB at N = 4096 and
        // 64 chains); without that memory, or with APM_FAR_LEFT=0, the two of the right-looking
        // schedule. The posterior bottom block borrows the first two (post_planes_of)
        const int npan = (c->nb + c->outer32 - 1) / c->outer32;
        const char* fl = getenv("APM_FAR_LEFT");
        if (npan > 2 && !(fl && atoi(fl) == 0)) {
            void* p = nullptr;
            if (hipMalloc(&p, sizeof(unsigned short) * npan * B * c->plane_cs) == hipSuccess) {
                c->allocs.push_back(p);
                c->planes = static_cast<unsigned short*>(p);
                c->plane_bufs = npan;
                c->far_left = true;
            } else {
                (void)hipGetLastError();
            }
        }
        if (!c->planes) c->planes = dalloc<unsigned short>(c, 2 * B * c->plane_cs);
        c->zt = dalloc<float>(c, B * 3 * 512 * 512);
        c->zplanes = dalloc<unsigned short>(c, B * 2 * 16 * 512 * 32);
    }
    // + 3: the bounded-spin timeouts of the dataflow panel (APM_PROF_DF_TIMEOUTS) and of the
    // TRSV (APM_PROF_TRSV_TIMEOUTS), the arrival-ticket counter (spin_words)
    c->dfprog = dalloc<unsigned long long>(c, (size_t)B * (c->nb + 1) + 3);
    HIPC(hipMemset(c->dfprog, 0, sizeof(unsigned long long) * (B * (c->nb + 1) + 3)));
    // one block of BLK_FIELDS x B words (StageBlk), mirrored in pinned host memory and uploaded
    // with one copy: [i3: 3B int64][ca: B][cb: B][seeds: B][ctrs: B]
    c->d_i3 = dalloc<int64_t>(c, BLK_FIELDS * B);
    c->d_ca = reinterpret_cast<double*>(c->d_i3 + BLK_CA * B);
    c->d_cb = reinterpret_cast<double*>(c->d_i3 + BLK_CB * B);
    c->d_seeds = reinterpret_cast<uint64_t*>(c->d_i3 + BLK_SEEDS * B);
    c->d_ctrs = reinterpret_cast<uint64_t*>(c->d_i3 + BLK_CTRS * B);
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&c->hblk), sizeof(int64_t) * BLK_FIELDS * B,
                       hipHostMallocDefault));
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&c->hth),
                       sizeof(double) * (size_t)B * std::max(c->P, 1), hipHostMallocDefault));
    c->U64 = dalloc<double>(c, n * S);
    const int64_t Lsz = (np + 64) * np;
    c->Sl = SlotSet{dalloc<float>(c, n_slots * Lsz), dalloc<double>(c, n_slots * np),
                    dalloc<double>(c, n_slots * np), dalloc<double>(c, n_slots * np),
                    dalloc<double>(c, n_slots), Lsz, np,
                    nullptr, dalloc<double>(c, n_slots * np), dalloc<int>(c, n_slots),
                    dalloc<int>(c, B), APM_WIDE_Q, APM_POST32_Q};
    c->l64_d = dalloc<double*>(c, n_slots);
    c->Sl.L64 = c->l64_d;
    c->l64_h.assign((size_t)n_slots, nullptr);
    HIPC(hipMemset(c->l64_d, 0, sizeof(double*) * n_slots));
    if (const char* e = getenv("APM_WIDE_Q")) c->Sl.wide_q = atof(e);  // development knob
    if (const char* e = getenv("APM_POST32_Q")) c->Sl.post_q = atof(e);
    c->Sl.post_q = std::min(c->Sl.post_q, c->Sl.wide_q);  // (a wide slot needs the fp64 factor)
    c->Sl.icm_thr = c->icm_thr;
    HIPC(hipMemset(c->Sl.cst, 0, sizeof(double) * n_slots));
    HIPC(hipMemset(c->Sl.wide, 0, sizeof(int) * n_slots));
    c->slot_wide.assign((size_t)n_slots, 0);
    c->slot_failed.assign((size_t)n_slots, 0);
    c->Up = UPool{dalloc<double>(c, n_ubufs * np * c->sp), np * c->sp, c->sp,
                  dalloc<float>(c, n_ubufs * np * c->sp)};
    HIPC(hipMemset(c->Up.base, 0, sizeof(double) * n_ubufs * np * c->sp));
    HIPC(hipMemset(c->Up.base32, 0, sizeof(float) * n_ubufs * np * c->sp));
}

void standalone_ctx(apm_ctx*& c, int device, int64_t n, const double* y) {
    if (!c) {
        c = new apm_ctx();
        init_ctx(c, device, APM_KERNEL_PRECOMPUTED, nullptr, n, 0, 0, y, 1e-8, 1, 1, 1, 1);
    } else {
        HIPC(hipSetDevice(device));
        std::vector<double> yp((size_t)c->np, 0.0);
        for (int64_t i = 0; i < n; ++i) yp[i] = y[i];
        HIPC(hipMemcpyAsync(c->y, yp.data(), sizeof(double) * c->np, hipMemcpyHostToDevice,
                            c->stream));
    }
}

void free_ctx(apm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // every stream drained before its buffers go (stream2 / stream3 work is joined into the main
    // stream by every call, but a call that threw may have left some behind)
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->stream3) (void)hipStreamSynchronize(c->stream3);
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->hpin) (void)hipHostFree(c->hpin);
    if (c->hblk) (void)hipHostFree(c->hblk);
    if (c->hth) (void)hipHostFree(c->hth);
    if (c->hx) (void)hipHostFree(c->hx);
    if (c->hmask) (void)hipHostFree(c->hmask);
    for (hipEvent_t e : c->evpool) (void)hipEventDestroy(e);
    if (c->stream3) (void)hipStreamDestroy(c->stream3);
    for (hipEvent_t* e : c->ev.all())
        if (*e) (void)hipEventDestroy(*e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    delete c;
}

}  // namespace apm_host
