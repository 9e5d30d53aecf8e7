// ebvo_capi.hip -- the C ABI of include/ebvo_hip.h: context and slots, host-buffer entry points,
// the sync-free device-resident stereo pipeline, profiling.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>

#include "ebvo_internal.h"

const char *const g_kernel_names[K_NUM] = {
    "toed_conv",   "toed_nms",   "toed_rowscan", "toed_compact", "toed_finalize", "toed_exact_centre", "toed_exact_mags", "cand_boxes", "epi_lines",
    "cand_count",  "scan",       "cand_fill",    "edge_patches", "ncc_pairs",     "ncc_stored", "misc", "sobel", "gn_refine", "sift",
    "gt_misc",     "gt_pool",    "gt_census",    "gt_rows",      "tgt_project",   "tgt_veridical", "tgt_rows",
    "pose_cascade", "tgt_grid_rows"};

// ------------------------------------------------------------------------------------------
int ebvo_fail_hip(ebvo_ctx *ctx, hipError_t e, const char *what, const char *file, int line)
{
    char buf[512];
    snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    if (ctx)
        ctx->last_error = buf;
    else
        fprintf(stderr, "[ebvo] %s\n", buf);
    (void)hipGetLastError();
    return EBVO_ERR_HIP;
}

int ebvo_grow(ebvo_ctx *ctx, Slot &s, GrowBuf &b, size_t bytes, bool bump_generation)
{
    if (bytes <= b.bytes && b.p)
        return EBVO_OK;
    // the stream may still be using the old allocation
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    if (b.p)
        (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    const size_t want = bytes + bytes / 4 + 256;
    if (bump_generation)
        ++s.buf_gen; // a captured chain of this slot may hold the old address
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess)
    {
        (void)hipGetLastError();
        ctx->last_error = "hipMalloc failed (out of device memory)";
        return EBVO_ERR_NOMEM;
    }
    b.bytes = want;
    return EBVO_OK;
}

bool ebvo_prof_begin(ebvo_ctx *ctx, Slot &s, int kid)
{
    if (!ctx->prof || !s.prof_now || (ctx->prof_only >= 0 && kid != ctx->prof_only))
        return false;
    ProfEvent pe;
    if (!ctx->prof_free.empty())
    {
        pe = ctx->prof_free.back();
        ctx->prof_free.pop_back();
    }
    else
    {
        if (hipEventCreate(&pe.a) != hipSuccess || hipEventCreate(&pe.b) != hipSuccess)
            return false;
    }
    pe.kid = kid;
    (void)hipEventRecord(pe.a, s.stream);
    s.prof_pending.push_back(pe);
    return true;
}

// Events for ONE kernel launch timed by its own dispatch (hipExtLaunchKernelGGL stamps them with the kernel's begin and
// end, the timestamps a kernel trace reports) instead of a pair recorded around the launch.  False when profiling is off.
bool ebvo_prof_kernel(ebvo_ctx *ctx, Slot &s, int kid, hipEvent_t *a, hipEvent_t *b)
{
    if (!ctx->prof || !s.prof_now || (ctx->prof_only >= 0 && kid != ctx->prof_only))
        return false;
    ProfEvent pe;
    if (!ctx->prof_free.empty())
    {
        pe = ctx->prof_free.back();
        ctx->prof_free.pop_back();
    }
    else
    {
        if (hipEventCreate(&pe.a) != hipSuccess || hipEventCreate(&pe.b) != hipSuccess)
            return false;
    }
    pe.kid = kid;
    s.prof_pending.push_back(pe);
    *a = pe.a;
    *b = pe.b;
    return true;
}

void ebvo_prof_end(ebvo_ctx *ctx, Slot &s)
{
    if (!ctx->prof || !s.prof_now || s.prof_pending.empty())
        return;
    (void)hipEventRecord(s.prof_pending.back().b, s.stream);
}

static int prof_drain(ebvo_ctx *ctx)
{
    for (Slot *sp : ctx->slots)
    {
        Slot &s = *sp;
        if (s.prof_pending.empty())
            continue;
        EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
        for (ProfEvent &pe : s.prof_pending)
        {
            float ms = 0;
            if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess)
            {
                ctx->prof_ms[pe.kid] += ms;
                ctx->prof_launches[pe.kid] += 1;
            }
            ctx->prof_free.push_back(pe);
        }
        s.prof_pending.clear();
    }
    return EBVO_OK;
}

static void free_buf(GrowBuf &b)
{
    if (b.p)
        (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

static void slot_destroy(Slot *s)
{
    if (!s)
        return;
    if (s->own_stream) // (a pair still running on a lane is drained by ebvo_ctx_destroy before any slot goes)
        (void)hipStreamSynchronize(s->own_stream);
    if (s->pair_graph)
        (void)hipGraphExecDestroy(s->pair_graph);
    for (ProfEvent &pe : s->prof_pending)
    {
        (void)hipEventDestroy(pe.a);
        (void)hipEventDestroy(pe.b);
    }
    for (int k = 0; k < 2; ++k)
    {
        ImageWS &ws = s->im[k];
        (void)hipFree(ws.img_base);
        (void)hipFree(ws.pix2);
        (void)hipFree(ws.raw_base);
        (void)hipFree(ws.undist_xs);
        (void)hipFree(ws.maps);
        (void)hipFree(ws.flag);
        (void)hipFree(ws.row_cnt);
        (void)hipFree(ws.row_off);
        (void)hipFree(ws.counts);
        (void)hipFree(ws.src);
        (void)hipFree(ws.edges);
        (void)hipFree(ws.all4);
        (void)hipFree(ws.cand_rec);
        (void)hipFree(ws.cand_flag);
        (void)hipFree(ws.cand_off);
        (void)hipFree(ws.cand_data);
        (void)hipFree(ws.cand_lists);
        (void)hipFree(ws.cand_lcount);
    }
    GrowBuf *bufs[] = {&s->lines,        &s->boxes_chunk,  &s->boxes_group,    &s->cand_cnt,       &s->cand_stage, &s->cand_tileflag, &s->cand_tiletot, &s->row_ptr, &s->grad_x, &s->grad_y, &s->gn_xy, &s->gn_out, &s->gn_valid, &s->gn_iters, &s->gn_state, &s->gn_lists, &s->gn_pack, &s->sift_used, &s->sift_img, &s->sift_desc, &s->sift_f32, &s->sift_dist, &s->tq_i32, &s->tq_cols, &s->tq_f64, &s->tq_u8, &s->tq_cells, &s->tq_chain, &s->fin_i32, &s->fin_edges, &s->fin_f64, &s->fin_u8, &s->fin_out,
                       &s->scan_tmp,     &s->col_idx,      &s->rc_edges,       &s->sims,           &s->best,
                       &s->keep,         &s->patches_raw,  &s->patches_norm,   &s->patches_flag,   &s->patches_norm_r,
                       &s->patches_flag_r, &s->pair_left,  &s->sincos,         &s->scratch_b,      &s->scratch_c,
                       &s->scratch_d,    &s->fetch_pack,   &s->pose_in,        &s->pose_geom,      &s->pose_order,
                       &s->pose_draw,    &s->pose_hyp,       &s->pose_sel,       &s->pose_casc,       &s->pose_refit,     &s->host_up,        &s->align_ws,       &s->depth_ws,       &s->carry_ws,       &s->cover_ws,       &s->gt_disp,       &s->gt_geom,        &s->gt_flags,
                       &s->gt_boxes,     &s->gt_pool_i32,  &s->gt_pool_idx,    &s->gt_rows,        &s->gt_tot,
                       &s->tgt_geom,     &s->tgt_i32,      &s->tgt_idx,        &s->tgt_u8,
                       &s->tgt_rows,     &s->tgt_flags,    &s->tgt_tot,
                       &s->tq_prior_geom, &s->tq_prior_live};
    for (GrowBuf *b : bufs)
        free_buf(*b);
    (void)hipFree(s->d_total);
    (void)hipFree(s->d_matches);
    (void)hipFree(s->d_sizes);
    (void)hipFree(s->d_F);
    (void)hipFree(s->d_result);
    if (s->h_result)
        (void)hipHostFree(s->h_result);
    if (s->h_arena)
        (void)hipHostFree(s->h_arena);
    if (s->ev_done)
        (void)hipEventDestroy(s->ev_done);
    if (s->ev_rebind)
        (void)hipEventDestroy(s->ev_rebind);
    if (s->ev_upload)
        (void)hipEventDestroy(s->ev_upload);
    if (s->h_push)
        (void)hipHostFree(s->h_push);
    if (s->h_mail)
        (void)hipHostFree(s->h_mail);
    if (s->h_up)
        (void)hipHostFree(s->h_up);
    (void)hipFree(s->d_fin_tot);
    if (s->h_fin_tot)
        (void)hipHostFree(s->h_fin_tot);
    if (s->ev_fin)
        (void)hipEventDestroy(s->ev_fin);
    (void)hipFree(s->d_tq_tot);
    if (s->h_tq_tot)
        (void)hipHostFree(s->h_tq_tot);
    if (s->ev_tq)
        (void)hipEventDestroy(s->ev_tq);
    if (s->own_stream)
        (void)hipStreamDestroy(s->own_stream);
    delete s;
}

// Result copies of ebvo_stereo_fetch_begin run on the context's copy stream: an entry point that writes buffers of the
// slot lets them finish first (the views stay valid; ebvo_stereo_fetch_end then returns at once).
static int drain_fetch(ebvo_ctx *ctx, Slot &s)
{
    if (s.fetch_pending)
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_rebind));
    if (s.upload_pending) // an asynchronous upload (ebvo_stereo_upload_async) still writes the slot's image buffers
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_upload));
    s.upload_pending = false;
    return EBVO_OK;
}

// an earlier stream-form upload of the slot must have landed before the mailbox names other images (host wait; rare)
static int drain_stream_upload(ebvo_ctx *ctx, Slot &s)
{
    if (s.upload_pending)
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_upload));
    s.upload_pending = false;
    return EBVO_OK;
}

static int slot_create(ebvo_ctx *ctx, Slot **out)
{
    Slot *s = new (std::nothrow) Slot();
    if (!s)
        return EBVO_ERR_NOMEM;
#define CK(call)                                                                   \
    do                                                                             \
    {                                                                              \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess)                                                      \
        {                                                                          \
            ebvo_fail_hip(ctx, e_, #call, __FILE__, __LINE__);                     \
            slot_destroy(s);                                                       \
            return e_ == hipErrorOutOfMemory ? EBVO_ERR_NOMEM : EBVO_ERR_HIP;      \
        }                                                                          \
    } while (0)
    CK(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    s->stream = s->own_stream;
    CK(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&s->ev_rebind, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&s->ev_upload, hipEventDisableTiming));
    const size_t H2 = 2 * (size_t)ctx->max_h, W2 = 2 * (size_t)ctx->max_w, np2 = H2 * W2;
    for (int k = 0; k < 2; ++k)
    {
        ImageWS &ws = s->im[k];
        CK(hipMalloc(&ws.img_base, (size_t)ctx->max_h * ctx->max_w + 128));
        // on the slot's own stream: hipMemset runs asynchronously on the NULL stream, which a non-blocking stream does
        // not wait for -- the zero fill could land after the first upload of a fresh context
        CK(hipMemsetAsync(ws.img_base, 0, (size_t)ctx->max_h * ctx->max_w + 128, s->stream));
        ws.img = ws.img_base + 64;
        CK(hipMalloc(&ws.pix2, sizeof(uint16_t) * ((size_t)ctx->max_h * ctx->max_w + 64)));
        CK(hipMemsetAsync(ws.pix2, 0, sizeof(uint16_t) * ((size_t)ctx->max_h * ctx->max_w + 64), s->stream));
        CK(hipMalloc(&ws.undist_xs, sizeof(double) * (size_t)ctx->max_w));
        if (ctx->undist_on)
        {
            CK(hipMalloc(&ws.raw_base, (size_t)ctx->max_h * ctx->max_w + 128));
            CK(hipMemsetAsync(ws.raw_base, 0, (size_t)ctx->max_h * ctx->max_w + 128, s->stream));
            ws.raw = ws.raw_base + 64;
        }
        CK(hipMalloc(&ws.maps, sizeof(double) * np2 * PL_NUM));
        CK(hipMalloc(&ws.flag, np2));
        CK(hipMalloc(&ws.row_cnt, sizeof(int32_t) * 2 * H2));
        CK(hipMalloc(&ws.row_off, sizeof(int32_t) * 3 * (H2 + 1)));
        CK(hipMalloc(&ws.counts, sizeof(int32_t) * 8));
        CK(hipMemsetAsync(ws.counts, 0, sizeof(int32_t) * 8, s->stream));
        CK(hipMalloc(&ws.cand_rec, 40 * (size_t)ctx->cap_edges));
        CK(hipMalloc(&ws.cand_flag, sizeof(int32_t) * 2 * (size_t)ctx->cap_edges));
        CK(hipMalloc(&ws.cand_off, sizeof(int32_t) * 2 * ((size_t)ctx->cap_edges + 1)));
        CK(hipMalloc(&ws.cand_data, 64 * (size_t)ctx->cap_edges));
        CK(hipMalloc(&ws.cand_lists, sizeof(int32_t) * 12 * (size_t)ctx->cap_edges));
        CK(hipMalloc(&ws.cand_lcount, sizeof(int32_t) * 12));
        CK(hipMalloc(&ws.src, sizeof(int32_t) * 2 * (size_t)ctx->cap_edges));
        CK(hipMalloc(&ws.edges, sizeof(ebvo_edge) * (size_t)ctx->cap_edges));
        CK(hipMalloc(&ws.all4, sizeof(double) * 4 * (size_t)ctx->cap_edges));
    }
    CK(hipMalloc(&s->d_total, sizeof(unsigned long long) * (1 + EBVO_TOTAL_PARTS)));
    CK(hipMalloc(&s->d_matches, sizeof(int32_t) * EBVO_MATCH_PARTS));
    CK(hipMalloc(&s->d_sizes, sizeof(int32_t) * 4));
    CK(hipMalloc(&s->d_F, sizeof(double) * 9));
    CK(hipHostMalloc(reinterpret_cast<void **>(&s->h_mail), sizeof(Slot::PullMail)));
    memset(s->h_mail, 0, sizeof(Slot::PullMail));
    CK(hipHostGetDevicePointer(reinterpret_cast<void **>(&s->d_mail), s->h_mail, 0));
    CK(hipMalloc(&s->d_result, sizeof(PairResult)));
    CK(hipHostMalloc(&s->h_result, sizeof(PairResult)));
    CK(hipHostGetDevicePointer(reinterpret_cast<void **>(&s->d_result_host), s->h_result, 0));
    CK(hipMalloc(&s->d_fin_tot, sizeof(int32_t) * 8));
    CK(hipHostMalloc(&s->h_fin_tot, sizeof(int32_t) * 8));
    CK(hipEventCreateWithFlags(&s->ev_fin, hipEventDisableTiming));
    CK(hipMalloc(&s->d_tq_tot, sizeof(unsigned long long) * 2));
    CK(hipHostMalloc(&s->h_tq_tot, sizeof(unsigned long long) * 2));
    CK(hipEventCreateWithFlags(&s->ev_tq, hipEventDisableTiming));
    CK(hipStreamSynchronize(s->stream));
#undef CK
    *out = s;
    return EBVO_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" const char *ebvo_strerror(int status)
{
    switch (status)
    {
    case EBVO_OK: return "ok";
    case EBVO_ERR_ARG: return "invalid argument";
    case EBVO_ERR_CAPACITY: return "output capacity too small";
    case EBVO_ERR_HIP: return "HIP runtime error";
    case EBVO_ERR_NOMEM: return "out of memory";
    case EBVO_ERR_STATE: return "call made in the wrong state";
    default: return "unknown status";
    }
}

extern "C" const char *ebvo_last_error(const ebvo_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

extern "C" int ebvo_abi_version(void) { return EBVO_ABI_VERSION; }

extern "C" int ebvo_set_toed_mode(ebvo_ctx *ctx, int mode)
{
    if (!ctx || (mode != EBVO_TOED_STRICT && mode != EBVO_TOED_HYBRID))
        return EBVO_ERR_ARG;
    ++ctx->graph_gen;
    ctx->toed_mode = mode;
    return EBVO_OK;
}

extern "C" int ebvo_get_toed_mode(const ebvo_ctx *ctx) { return ctx ? ctx->toed_mode : EBVO_ERR_ARG; }

extern "C" int64_t ebvo_toed_fallbacks(const ebvo_ctx *ctx) { return ctx ? ctx->toed_fallbacks : -1; }

extern "C" int64_t ebvo_graph_launches(const ebvo_ctx *ctx) { return ctx ? ctx->graph_launches : -1; }

extern "C" int ebvo_toed_stats(ebvo_ctx *ctx, int slot, int32_t out[8])
{
    if (!ctx || !out || slot < 0 || slot >= (int)ctx->slots.size())
        return EBVO_ERR_ARG;
    Slot &s = *ctx->slots[(size_t)slot];
    if (s.in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < 2; ++k)
        EBVO_HIP(ctx, hipMemcpyAsync(out + 4 * k, s.im[k].counts, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    return EBVO_OK;
}

extern "C" void ebvo_ctx_destroy(ebvo_ctx *ctx)
{
    if (!ctx)
        return;
    (void)hipSetDevice(ctx->device);
    for (hipStream_t st : ctx->lane_streams) // pairs still running on a lane use the buffers of their slot
        (void)hipStreamSynchronize(st);
    if (ctx->copy_stream)
        (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->upload_stream)
        (void)hipStreamSynchronize(ctx->upload_stream);
    for (Slot *s : ctx->slots)
        slot_destroy(s);
    if (ctx->upload_stream)
        (void)hipStreamDestroy(ctx->upload_stream);
    for (const ebvo_ctx::HostRange &r : ctx->host_ranges) // (the caller should have unregistered them)
        if (r.ours)
            (void)hipHostUnregister(const_cast<uint8_t *>(r.host));
    for (hipStream_t st : ctx->lane_streams)
        (void)hipStreamDestroy(st);
    if (ctx->copy_stream)
        (void)hipStreamDestroy(ctx->copy_stream);
    for (ProfEvent &pe : ctx->prof_free)
    {
        (void)hipEventDestroy(pe.a);
        (void)hipEventDestroy(pe.b);
    }
    (void)hipFree(ctx->kf_L);
    (void)hipFree(ctx->kf_R);
    (void)hipFree(ctx->kf_Ln);
    (void)hipFree(ctx->kf_Rn);
    (void)hipFree(ctx->kf_Lf);
    (void)hipFree(ctx->kf_Ld);
    (void)hipFree(ctx->kf_Rd);
    (void)hipFree(ctx->kf_imgL);
    (void)hipFree(ctx->kf_imgR);
    (void)hipFree(ctx->kf_Rf);
    for (void *p : {(void *)ctx->kf_lambda_alt, (void *)ctx->kf_info_alt, (void *)ctx->kf_nobs_alt, (void *)ctx->kf_dflags_alt,
                    (void *)ctx->kf_src, (void *)ctx->kf_src_alt})
        (void)hipFree(p);
    (void)hipFree(ctx->kf_lambda);
    (void)hipFree(ctx->kf_info);
    (void)hipFree(ctx->kf_nobs);
    (void)hipFree(ctx->kf_dflags);
    for (PinnedBuf *b : {&ctx->sw_toed[0], &ctx->sw_toed[1], &ctx->sw_cand, &ctx->sw_ncc, &ctx->sw_up})
        if (b->p)
            (void)hipHostFree(b->p);
    delete ctx;
}

extern "C" int ebvo_ctx_create(int device, int max_h, int max_w, ebvo_ctx **out)
{
    if (!out || max_h < 32 || max_w < 32 || (int64_t)max_h * max_w > (1ll << 28))
        return EBVO_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return ebvo_fail_hip(nullptr, e == hipSuccess ? hipErrorNoDevice : e, "hipGetDeviceCount (no HIP device)",
                             __FILE__, __LINE__);
    if (device < 0 || device >= ndev)
        return EBVO_ERR_ARG;
    ebvo_ctx *ctx = new (std::nothrow) ebvo_ctx();
    if (!ctx)
        return EBVO_ERR_NOMEM;
    ctx->device = device;
    ctx->max_h = max_h;
    ctx->max_w = max_w;
    ctx->cap_edges = max_h * max_w;
    {
        // both modes return the same bits (every TOED parity test runs in both); hybrid does a third of the work
        const char *m = getenv("EBVO_TOED_MODE");
        ctx->toed_mode = (m && strcmp(m, "strict") == 0) ? EBVO_TOED_STRICT : EBVO_TOED_HYBRID;
        const char *g = getenv("EBVO_GRAPHS"); // "0": the pair chain as direct launches (hipGraph capture is the default)
        ctx->use_graphs = (g && strcmp(g, "0") == 0) ? 0 : 1;
    }
    int rc;
    auto fail = [&](int code) {
        fprintf(stderr, "[ebvo] ebvo_ctx_create: %s (%s)\n", ebvo_strerror(code), ctx->last_error.c_str());
        ebvo_ctx_destroy(ctx);
        return code;
    };
    if (hipSetDevice(device) != hipSuccess)
        return fail(EBVO_ERR_HIP);
    Slot *s0 = nullptr;
    if ((rc = slot_create(ctx, &s0)))
        return fail(rc);
    ctx->slots.push_back(s0);
    if ((rc = toed_init_constants(ctx)))
        return fail(rc);
    *out = ctx;
    return EBVO_OK;
}

static int check_size(ebvo_ctx *ctx, int h, int w)
{
    if (h < 32 || w < 32 || h > ctx->max_h || w > ctx->max_w)
    {
        ctx->last_error = "image size outside [32, ctx maximum]";
        return EBVO_ERR_ARG;
    }
    return EBVO_OK;
}

static int upload_image(ebvo_ctx *ctx, Slot &s, int k, const uint8_t *img, int h, int w, ptrdiff_t stride, bool to_raw = false,
                        hipStream_t on = nullptr)
{
    if (stride < w)
        return EBVO_ERR_ARG;
    uint8_t *dst = to_raw ? s.im[k].raw : s.im[k].img;
    const hipStream_t st = on ? on : s.stream;
    // a tightly packed image is ONE linear copy: the 2-D copy of pageable memory is staged row by row (measured 3 ms
    // per KITTI image against 0.1 ms)
    if (stride == (ptrdiff_t)w)
        EBVO_HIP(ctx, hipMemcpyAsync(dst, img, (size_t)w * h, hipMemcpyHostToDevice, st));
    else
        EBVO_HIP(ctx, hipMemcpy2DAsync(dst, (size_t)w, img, (size_t)stride, (size_t)w, (size_t)h,
                                       hipMemcpyHostToDevice, st));
    return EBVO_OK;
}

// host-buffer entry points use slot 0; they must not run while a submitted pair is in flight on it
static int host_slot(ebvo_ctx *ctx, Slot **out)
{
    Slot &s = *ctx->slots[0];
    if (s.in_flight || s.fin_in_flight || s.tq_in_flight)
    {
        ctx->last_error = "slot 0 has submitted work in flight; call ebvo_stereo_wait / ebvo_stereo_finalize_wait / ebvo_temporal_match_wait first";
        return EBVO_ERR_STATE;
    }
    if (int rc = drain_fetch(ctx, s)) // result copies of the previous pair (copy stream) still read the slot's buffers
        return rc;
    s.fetch_pending = false;
    s.have_pair = s.have_run = s.have_refined = s.have_final = false;
    s.gt_armed = false; // the ground truth was given for the pair that ran
    s.sift_left_valid = false;
    s.undist_pair = false;
    s.fetch_what = 0;
    *out = &s;
    return EBVO_OK;
}

// ---- host-array calls: copies between a caller's arrays and a carved device buffer ----------------------------------------
// Nothing is copied for an empty array or a null host pointer (an optional argument the caller left out).
static int copy_up(ebvo_ctx *ctx, hipStream_t st, void *dst_dev, const void *src_host, size_t bytes)
{
    if (bytes && src_host)
        EBVO_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, st));
    return EBVO_OK;
}

static int copy_down(ebvo_ctx *ctx, hipStream_t st, void *dst_host, const void *src_dev, size_t bytes)
{
    if (bytes && dst_host)
        EBVO_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
    return EBVO_OK;
}

// The host-array calls run on slot 0's stream with a buffer of their own (host_up): the slot's pair, its results and its
// armed state stay as they are (unlike host_slot(), whose callers reuse the pair's buffers).
static int gt_host_slot(ebvo_ctx *ctx, Slot **out)
{
    Slot &s = *ctx->slots[0];
    if (s.in_flight || s.fin_in_flight || s.tq_in_flight)
    {
        ctx->last_error = "slot 0 has submitted work in flight; call ebvo_stereo_wait / ebvo_stereo_finalize_wait / ebvo_temporal_match_wait first";
        return EBVO_ERR_STATE;
    }
    *out = &s;
    return EBVO_OK;
}

// One host-array call.  It sets the device, takes slot 0 and copies on the slot's stream.  The copies read and write the
// caller's arrays and the function's locals, so none of them may outlive the call: finish() waits for them, and the
// destructor does on every return that did not get there.  A local that down() writes into is declared before this object.
// Two kinds: STAGED leaves the slot's pair alone (gt_host_slot) and works in the carved staging buffer, stage() / at();
// PAIR_BUFFERS gives the pair up (host_slot) and works in the pair's named buffers, grow() / image(), because the stage
// enqueues it calls write into slot-owned buffers.
namespace
{
struct HostCall
{
    enum Kind { STAGED, PAIR_BUFFERS };
    ebvo_ctx *ctx;
    Slot *s = nullptr;
    int rc;               // the device and the slot's state first, then the first failure of a helper; every helper returns it
    bool pending = false; // copies were enqueued since the last finish()

    explicit HostCall(ebvo_ctx *c, Kind kind = STAGED) : ctx(c)
    {
        const hipError_t e = hipSetDevice(c->device);
        rc = e != hipSuccess      ? ebvo_fail_hip(c, e, "hipSetDevice(ctx->device)", __FILE__, __LINE__)
             : kind == PAIR_BUFFERS ? host_slot(c, &s)
                                    : gt_host_slot(c, &s);
    }
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    ~HostCall()
    {
        if (pending)
            (void)hipStreamSynchronize(s->stream);
    }

    Slot &slot() const { return *s; }
    // the staging buffer holds L.total() bytes; at<T>(offset) is an array of it
    int stage(const Carve &L) { return rc ? rc : (rc = ebvo_grow(ctx, *s, s->host_up, L.total(), false)); }
    template <class T> T *at(size_t offset) const { return (T *)((char *)s->host_up.p + offset); }
    // a named buffer of the pair (a captured chain may hold its old address: the generation is bumped)
    int grow(GrowBuf &b, size_t bytes) { return rc ? rc : (rc = ebvo_grow(ctx, *s, b, bytes)); }

    int up(void *dst_dev, const void *src_host, size_t bytes)
    {
        pending = true;
        return rc ? rc : (rc = copy_up(ctx, s->stream, dst_dev, src_host, bytes));
    }
    // `rows` rows of row_bytes each, src_pitch bytes apart on the host, packed on the device
    int up_rows(void *dst_dev, const void *src_host, size_t row_bytes, size_t src_pitch, size_t rows)
    {
        pending = true;
        if (rc)
            return rc;
        const hipError_t e = hipMemcpy2DAsync(dst_dev, row_bytes, src_host, src_pitch, row_bytes, rows, hipMemcpyHostToDevice, s->stream);
        return e == hipSuccess ? rc : (rc = ebvo_fail_hip(ctx, e, "hipMemcpy2DAsync(dst_dev, src_host)", __FILE__, __LINE__));
    }
    // image k of the slot (upload_image: one linear copy for a packed image)
    int image(int k, const uint8_t *img, int h, int w, ptrdiff_t stride)
    {
        pending = true;
        return rc ? rc : (rc = upload_image(ctx, *s, k, img, h, w, stride));
    }
    int down(void *dst_host, const void *src_dev, size_t bytes)
    {
        pending = true;
        return rc ? rc : (rc = copy_down(ctx, s->stream, dst_host, src_dev, bytes));
    }
    // `rows` packed rows of row_bytes each on the device, dst_pitch bytes apart on the host (one linear copy if that is packed too)
    int down_rows(void *dst_host, size_t dst_pitch, const void *src_dev, size_t row_bytes, size_t rows)
    {
        if (dst_pitch == row_bytes)
            return down(dst_host, src_dev, row_bytes * rows);
        pending = true;
        if (rc)
            return rc;
        const hipError_t e = hipMemcpy2DAsync(dst_host, dst_pitch, src_dev, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost, s->stream);
        return e == hipSuccess ? rc : (rc = ebvo_fail_hip(ctx, e, "hipMemcpy2DAsync(dst_host, src_dev)", __FILE__, __LINE__));
    }
    int fill(void *dst_dev, int byte, size_t bytes)
    {
        if (rc || !bytes)
            return rc;
        const hipError_t e = hipMemsetAsync(dst_dev, byte, bytes, s->stream);
        return e == hipSuccess ? rc : (rc = ebvo_fail_hip(ctx, e, "hipMemsetAsync(dst_dev, byte, bytes, stream)", __FILE__, __LINE__));
    }
    // wait for the stream whatever happened before; an earlier failure comes before the wait's own
    int finish()
    {
        pending = false;
        const hipError_t e = hipStreamSynchronize(s->stream);
        if (!rc && e != hipSuccess)
            rc = ebvo_fail_hip(ctx, e, "hipStreamSynchronize(stream)", __FILE__, __LINE__);
        return rc;
    }
};
} // namespace

// a CSR row_ptr of nL rows: starts at 0 and never decreases; *np: the listed total
static int check_csr(const int32_t *row_ptr, int nL, int64_t *np)
{
    if (nL < 0 || !row_ptr || row_ptr[0] != 0)
        return EBVO_ERR_ARG;
    for (int i = 0; i < nL; ++i)
        if (row_ptr[i + 1] < row_ptr[i])
            return EBVO_ERR_ARG;
    *np = row_ptr[nL];
    return EBVO_OK;
}

// run TOED on n_img resident images of the slot and read the counts back (synchronises)
namespace
{
struct EventTriple // destroyed on every return path
{
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~EventTriple()
    {
        for (hipEvent_t ev : e)
            if (ev)
                (void)hipEventDestroy(ev);
    }
};
} // namespace

static int toed_sync(ebvo_ctx *ctx, Slot &s, int n_img, int h, int w, float *ms_conv, float *ms_nms)
{
    EventTriple ev;
    const bool timed = ms_conv || ms_nms;
    if (timed)
        for (hipEvent_t &e : ev.e)
            EBVO_HIP(ctx, hipEventCreate(&e));
    // the counts travel through the slot's pinned record, never through this stack frame: a failure between the
    // enqueue of a copy and the synchronisation cannot leave a DMA pointing at dead memory
    int32_t *hc = reinterpret_cast<int32_t *>(s.h_result);
    static_assert(sizeof(PairResult) >= 6 * sizeof(int32_t), "pinned record too small for the TOED counts");
    int mode = ctx->toed_mode;
    for (int attempt = 0; attempt < 2; ++attempt)
    {
        int rc = toed_enqueue(ctx, s, n_img, h, w, ev.e[0], ev.e[1], ev.e[2], mode);
        if (rc)
            return rc;
        hipError_t e = hipSuccess;
        for (int k = 0; k < n_img && e == hipSuccess; ++k)
        {
            e = hipMemcpyAsync(hc + 3 * k, s.im[k].counts, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(hc + 3 * k + 2, s.im[k].counts + 4, sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
        }
        const hipError_t es = hipStreamSynchronize(s.stream); // also on failure: nothing may stay in flight
        if (e != hipSuccess || es != hipSuccess)
            return ebvo_fail_hip(ctx, e != hipSuccess ? e : es, "TOED count read-back", __FILE__, __LINE__);
        bool fits = true;
        for (int k = 0; k < n_img; ++k)
        {
            s.im[k].n_total = hc[3 * k];
            s.im[k].n_kept = hc[3 * k + 1];
            if (mode == EBVO_TOED_HYBRID && hc[3 * k + 2] > ctx->cap_edges)
                fits = false;
        }
        if (fits)
            break;
        // the screen flagged more grid points than the candidate buffers hold (an image of ties): the strict path has no
        // candidate lists and handles any image
        mode = EBVO_TOED_STRICT;
        ++ctx->toed_fallbacks;
    }
    if (timed)
    {
        float a = 0, b = 0;
        EBVO_HIP(ctx, hipEventElapsedTime(&a, ev.e[0], ev.e[1]));
        EBVO_HIP(ctx, hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
        if (ms_conv) *ms_conv = a;
        if (ms_nms) *ms_nms = b;
    }
    return EBVO_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" int ebvo_toed(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, ebvo_edge *out, int cap,
                         int *n_kept, int *n_total, double *all4, int cap_all, double *t_conv, double *t_nms)
{
    if (!ctx || !img || !n_kept || !n_total || cap < 0 || cap_all < 0 || (cap > 0 && !out))
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    ctx->sw_tag[0] = ctx->sw_tag[1] = 0; // the edge lists of the resident stage-wise calls live in these workspaces
    if (hc.image(0, img, h, w, stride))
        return hc.rc;
    float ms_c = 0, ms_n = 0;
    const bool timed = t_conv || t_nms;
    if (int rc = toed_sync(ctx, s, 1, h, w, timed ? &ms_c : nullptr, timed ? &ms_n : nullptr))
        return rc;
    const ImageWS &ws = s.im[0];
    *n_kept = ws.n_kept;
    *n_total = ws.n_total;
    if (t_conv) *t_conv = ms_c * 1e-3;
    if (t_nms) *t_nms = ms_n * 1e-3;
    if (ws.n_total > ctx->cap_edges)
    {
        ctx->last_error = "internal edge capacity exceeded";
        return EBVO_ERR_CAPACITY;
    }
    if ((out && ws.n_kept > cap) || (all4 && ws.n_total > cap_all))
        return EBVO_ERR_CAPACITY;
    hc.down(out, ws.edges, sizeof(ebvo_edge) * (size_t)ws.n_kept);
    hc.down(all4, ws.all4, sizeof(double) * 4 * (size_t)ws.n_total);
    return hc.finish();
}

extern "C" int ebvo_toed_screen_audit(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, ebvo_screen_audit *out)
{
    if (!ctx || !img || !out)
        return EBVO_ERR_ARG;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    Slot *sp;
    if ((rc = check_size(ctx, h, w)) || (rc = host_slot(ctx, &sp)))
        return rc;
    Slot &s = *sp;
    ctx->sw_tag[0] = ctx->sw_tag[1] = 0;
    if ((rc = upload_image(ctx, s, 0, img, h, w, stride)))
        return rc;
    ctx->screen_audit = true; // the next toed_enqueue keeps the screen's values and runs the audit kernel behind the exact stage
    rc = toed_enqueue(ctx, s, 1, h, w, nullptr, nullptr, nullptr, EBVO_TOED_HYBRID);
    ctx->screen_audit = false;
    // a diagnostic: drain the stream, then plain synchronous copies into this frame
    const hipError_t es = hipStreamSynchronize(s.stream);
    if (rc)
        return rc;
    EBVO_HIP(ctx, es);
    unsigned long long hw[6];
    int32_t hc[5];
    EBVO_HIP(ctx, hipMemcpy(hw, toed_screen_audit_result(s, 0, h, w), sizeof hw, hipMemcpyDeviceToHost));
    EBVO_HIP(ctx, hipMemcpy(hc, s.im[0].counts, sizeof hc, hipMemcpyDeviceToHost));
    if (hc[4] > ctx->cap_edges)
    {
        ctx->last_error = "the screen flagged more grid points than the context holds: nothing to audit";
        return EBVO_ERR_CAPACITY;
    }
    double b[5];
    toed_screen_budget(b);
    auto dbl = [](unsigned long long v) { double d; memcpy(&d, &v, sizeof d); return d; };
    out->n_maxima = hc[0];
    out->n_kept = hc[1];
    out->n_candidates = hc[2];
    out->n_neighbour_points = hc[3];
    out->max_err_gx = dbl(hw[0]);
    out->max_err_gy = dbl(hw[1]);
    out->max_err_mag = dbl(hw[2]);
    out->max_err_mag_neighbours = dbl(hw[3]);
    out->bound_g = b[0];
    out->bound_mag = b[1];
    out->bound_slope = b[2];
    out->tol_mag = b[3];
    out->tol_slope = b[4];
    return EBVO_OK;
}

extern "C" int ebvo_toed_pair(ebvo_ctx *ctx, const uint8_t *img_left, const uint8_t *img_right, int h, int w,
                              ptrdiff_t stride_left, ptrdiff_t stride_right, ebvo_edge *out_left,
                              ebvo_edge *out_right, int cap, int n_kept[2], int n_total[2])
{
    if (!ctx || !img_left || !img_right || !n_kept || !n_total || cap < 0)
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    ctx->sw_tag[0] = ctx->sw_tag[1] = 0;
    if (hc.image(0, img_left, h, w, stride_left) || hc.image(1, img_right, h, w, stride_right))
        return hc.rc;
    if (int rc = toed_sync(ctx, s, 2, h, w, nullptr, nullptr))
        return rc;
    ebvo_edge *outs[2] = {out_left, out_right};
    bool too_small = false;
    for (int k = 0; k < 2; ++k)
    {
        n_kept[k] = s.im[k].n_kept;
        n_total[k] = s.im[k].n_total;
        if (s.im[k].n_total > ctx->cap_edges)
            return EBVO_ERR_CAPACITY;
        if (outs[k] && s.im[k].n_kept > cap)
            too_small = true;
    }
    if (too_small)
        return EBVO_ERR_CAPACITY;
    for (int k = 0; k < 2; ++k)
        hc.down(outs[k], s.im[k].edges, sizeof(ebvo_edge) * (size_t)s.im[k].n_kept);
    return hc.finish();
}

extern "C" int ebvo_epipolar_lines(const double F[9], const ebvo_edge *edges, int n, double *lines)
{
    if (!F || (n > 0 && (!edges || !lines)) || n < 0)
        return EBVO_ERR_ARG;
    for (int k = 0; k < n; ++k)
        for (int r = 0; r < 3; ++r)
            lines[(size_t)k * 3 + r] = (F[r * 3 + 0] * edges[k].x + F[r * 3 + 1] * edges[k].y) + F[r * 3 + 2];
    return EBVO_OK;
}

// The thresholds every candidate search accepts: epi_thr, max_disp and orient_thr_deg in [0, +inf] (+inf: unbounded),
// ncc_thr any value but NaN.  A negative max_disp would pass s = 0 through the squared test (s < max_disp^2) although
// the reference's sqrt(0) <= max_disp fails; NaN would make every predicate false or the search box undefined.
static bool stereo_thresholds_ok(double epi_thr, double max_disp, double orient_thr_deg, double ncc_thr)
{
    return epi_thr >= 0 && max_disp >= 0 && orient_thr_deg >= 0 && ncc_thr == ncc_thr;
}

static int epi_candidates_impl(ebvo_ctx *ctx, const ebvo_edge *L, int nL, const ebvo_edge *R, int nR, const double *lines,
                               double epi_thr, double max_disp, double orient_thr_deg, int stage_mask, int32_t *row_ptr,
                               int32_t *col_idx, uint8_t *orient_ok, int64_t cap, int64_t *n_pairs);

extern "C" int ebvo_epi_candidates(ebvo_ctx *ctx, const ebvo_edge *L, int nL, const ebvo_edge *R, int nR,
                                   const double *lines, double epi_thr, double max_disp, double orient_thr_deg,
                                   int stage_mask, int32_t *row_ptr, int32_t *col_idx, int64_t cap,
                                   int64_t *n_pairs)
{
    return epi_candidates_impl(ctx, L, nL, R, nR, lines, epi_thr, max_disp, orient_thr_deg, stage_mask, row_ptr, col_idx, nullptr,
                               cap, n_pairs);
}

extern "C" int ebvo_epi_candidates_staged(ebvo_ctx *ctx, const ebvo_edge *L, int nL, const ebvo_edge *R, int nR,
                                          const double *lines, double epi_thr, double max_disp, double orient_thr_deg,
                                          int32_t *row_ptr, int32_t *col_idx, uint8_t *orient_ok, int64_t cap,
                                          int64_t *n_pairs)
{
    if (cap > 0 && !orient_ok)
        return EBVO_ERR_ARG;
    return epi_candidates_impl(ctx, L, nL, R, nR, lines, epi_thr, max_disp, orient_thr_deg,
                               EBVO_STAGE_EPIPOLAR | EBVO_STAGE_DISPARITY, row_ptr, col_idx, orient_ok, cap, n_pairs);
}

static int epi_candidates_impl(ebvo_ctx *ctx, const ebvo_edge *L, int nL, const ebvo_edge *R, int nR, const double *lines,
                               double epi_thr, double max_disp, double orient_thr_deg, int stage_mask, int32_t *row_ptr,
                               int32_t *col_idx, uint8_t *orient_ok, int64_t cap, int64_t *n_pairs)
{
    if (!ctx || nL < 0 || nR < 0 || !row_ptr || !n_pairs || cap < 0 || (cap > 0 && !col_idx) ||
        (nL > 0 && (!L || !lines)) || (nR > 0 && !R) || (stage_mask & ~EBVO_STAGE_ALL) || stage_mask == 0 ||
        !stereo_thresholds_ok(epi_thr, max_disp, orient_thr_deg, 0.0))
        return EBVO_ERR_ARG;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    *n_pairs = 0;
    if (nL == 0 || nR == 0)
    {
        memset(row_ptr, 0, sizeof(int32_t) * ((size_t)nL + 1));
        return EBVO_OK;
    }
    if (hc.grow(s.scratch_b, sizeof(ebvo_edge) * (size_t)nL) || hc.grow(s.scratch_c, sizeof(ebvo_edge) * (size_t)nR) ||
        hc.grow(s.lines, sizeof(double) * 3 * (size_t)nL) || hc.up(s.scratch_b.p, L, sizeof(ebvo_edge) * (size_t)nL) ||
        hc.up(s.lines.p, lines, sizeof(double) * 3 * (size_t)nL) || hc.up(s.scratch_c.p, R, sizeof(ebvo_edge) * (size_t)nR))
        return hc.rc;
    const ebvo_edge *dL = (const ebvo_edge *)s.scratch_b.p, *dR = (const ebvo_edge *)s.scratch_c.p;
    if (int rc = match_candidates_enqueue(ctx, s, dL, nL, nullptr, dR, nR, nullptr, 0, (const double *)s.lines.p, epi_thr,
                                          max_disp, orient_thr_deg, stage_mask, false))
        return rc;
    // the total lands in the slot's pinned record (not in this stack frame)
    unsigned long long *h_total_p = reinterpret_cast<unsigned long long *>(s.h_result);
    hc.down(h_total_p, s.d_total, sizeof(*h_total_p));
    hc.down(row_ptr, s.row_ptr.p, sizeof(int32_t) * ((size_t)nL + 1));
    if (hc.finish())
        return hc.rc;
    const unsigned long long h_total = *h_total_p;
    if (h_total > 0x7fffffffull)
    {
        ctx->last_error = "candidate list exceeds 2^31-1 pairs";
        return EBVO_ERR_CAPACITY;
    }
    const int64_t np = (int64_t)h_total;
    *n_pairs = np;
    if (np > cap)
        return (col_idx || cap > 0) ? EBVO_ERR_CAPACITY : EBVO_OK;
    if (np == 0 || !col_idx)
        return EBVO_OK;
    if (hc.grow(s.col_idx, sizeof(int32_t) * (size_t)np))
        return hc.rc;
    s.cap_pairs = np;
    if (int rc = match_candidates_fill_enqueue(ctx, s, dL, nL, nullptr, dR, nR, nullptr, 0, (const double *)s.lines.p,
                                               epi_thr, max_disp, orient_thr_deg, stage_mask))
        return rc;
    if (orient_ok)
    {
        // the third reference stage (apply_orientation_filter, src/Stereo_Matches.cpp:863-915) as one flag per listed pair
        if (hc.grow(s.keep, (size_t)np))
            return hc.rc;
        if (int rc = match_orient_flags_enqueue(ctx, s, dL, nL, dR, (const int32_t *)s.row_ptr.p, (const int32_t *)s.col_idx.p,
                                                np, orient_thr_deg, (uint8_t *)s.keep.p))
            return rc;
    }
    hc.down(col_idx, s.col_idx.p, sizeof(int32_t) * (size_t)np);
    hc.down(orient_ok, s.keep.p, (size_t)np);
    if (hc.finish())
        return hc.rc;
    s.cap_pairs = 0; // the pipeline re-establishes its own capacity
    return EBVO_OK;
}

extern "C" void ebvo_gn_default_params(ebvo_gn_params *p)
{
    if (!p)
        return;
    p->max_iter = EBVO_GN_MAX_ITER;
    p->tol = EBVO_GN_TOL;
    p->huber_delta = EBVO_GN_HUBER_DELTA;
}

extern "C" int ebvo_sobel_gradients(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, float *gx,
                                    float *gy)
{
    if (!ctx || !img || !gx || !gy)
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    const size_t bytes = sizeof(float) * (size_t)h * w;
    if (hc.image(0, img, h, w, stride) || hc.grow(s.grad_x, bytes) || hc.grow(s.grad_y, bytes))
        return hc.rc;
    if (int rc = refine_sobel_enqueue(ctx, s, s.im[0].img, h, w, w, (float *)s.grad_x.p, (float *)s.grad_y.p, nullptr))
        return rc;
    hc.down(gx, s.grad_x.p, bytes);
    hc.down(gy, s.grad_y.p, bytes);
    return hc.finish();
}

extern "C" int ebvo_gn_refine_stereo(ebvo_ctx *ctx, const uint8_t *imgL, const uint8_t *imgR, int h, int w,
                                     ptrdiff_t strideL, ptrdiff_t strideR, const ebvo_edge *L, int nL,
                                     const double *lines, const int32_t *row_ptr, const double *cand_xy,
                                     const ebvo_gn_params *params, double *alpha, double *score, double *confidence,
                                     uint8_t *validity, int32_t *iters, double *refined_xy)
{
    if (!ctx || !imgL || !imgR || nL < 0 || !row_ptr || !params || (nL > 0 && (!L || !lines)) || params->max_iter < 1 ||
        !(params->tol >= 0) || !(params->huber_delta > 0))
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    int64_t np = 0;
    if (check_csr(row_ptr, nL, &np))
        return EBVO_ERR_ARG;
    if (np == 0)
        return EBVO_OK;
    if (!cand_xy || !alpha || !score || !confidence || !validity || !iters || !refined_xy)
        return EBVO_ERR_ARG;
    const size_t npz = (size_t)np;
    if (hc.image(0, imgL, h, w, strideL) || hc.image(1, imgR, h, w, strideR) || hc.grow(s.scratch_b, sizeof(ebvo_edge) * (size_t)nL) ||
        hc.grow(s.lines, sizeof(double) * 3 * (size_t)nL) || hc.grow(s.row_ptr, sizeof(int32_t) * ((size_t)nL + 1)) ||
        hc.grow(s.pair_left, sizeof(int32_t) * npz) || hc.grow(s.gn_xy, sizeof(double) * 2 * npz) ||
        hc.grow(s.gn_out, sizeof(double) * 5 * npz) || hc.grow(s.gn_valid, npz) || hc.grow(s.gn_iters, sizeof(int32_t) * npz) ||
        hc.up(s.scratch_b.p, L, sizeof(ebvo_edge) * (size_t)nL) || hc.up(s.lines.p, lines, sizeof(double) * 3 * (size_t)nL) ||
        hc.up(s.row_ptr.p, row_ptr, sizeof(int32_t) * ((size_t)nL + 1)) || hc.up(s.gn_xy.p, cand_xy, sizeof(double) * 2 * npz))
        return hc.rc;
    double *out = (double *)s.gn_out.p;
    int rc;
    if ((rc = match_expand_rows_enqueue(ctx, s, (const int32_t *)s.row_ptr.p, nL, np, (int32_t *)s.pair_left.p)) ||
        (rc = refine_gn_stereo_enqueue(ctx, s, s.im[0].img, s.im[1].img, nullptr, h, w, (const ebvo_edge *)s.scratch_b.p, nL,
                                       (const double *)s.lines.p, (const int32_t *)s.pair_left.p,
                                       (const double *)s.gn_xy.p, nullptr, nullptr, nullptr, np, params->max_iter,
                                       params->tol, params->huber_delta,
                                       out, out + npz, out + 2 * npz, (uint8_t *)s.gn_valid.p, (int32_t *)s.gn_iters.p,
                                       out + 3 * npz)))
        return rc;
    hc.down(alpha, out, sizeof(double) * npz);
    hc.down(score, out + npz, sizeof(double) * npz);
    hc.down(confidence, out + 2 * npz, sizeof(double) * npz);
    hc.down(refined_xy, out + 3 * npz, sizeof(double) * 2 * npz);
    hc.down(validity, s.gn_valid.p, npz);
    hc.down(iters, s.gn_iters.p, sizeof(int32_t) * npz);
    return hc.finish();
}

extern "C" int ebvo_edge_patches(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride,
                                 const ebvo_edge *edges, int n, float *patches)
{
    if (!ctx || !img || n < 0 || (n > 0 && (!edges || !patches)))
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (n == 0)
        return EBVO_OK;
    if (hc.image(0, img, h, w, stride) || hc.grow(s.scratch_b, sizeof(ebvo_edge) * (size_t)n) ||
        hc.grow(s.patches_raw, sizeof(float) * 98 * (size_t)n) || hc.up(s.scratch_b.p, edges, sizeof(ebvo_edge) * (size_t)n))
        return hc.rc;
    if (int rc = match_patches_enqueue(ctx, s, s.im[0].img, h, w, w, (const ebvo_edge *)s.scratch_b.p, n, nullptr, 0,
                                       (float *)s.patches_raw.p, nullptr, nullptr))
        return rc;
    hc.down(patches, s.patches_raw.p, sizeof(float) * 98 * (size_t)n);
    return hc.finish();
}

extern "C" int ebvo_ncc_pairs(ebvo_ctx *ctx, const uint8_t *imgL, const uint8_t *imgR, int h, int w,
                              ptrdiff_t strideL, ptrdiff_t strideR, const ebvo_edge *L, int nL, const ebvo_edge *Rc,
                              const int32_t *row_ptr, double thr, float *left_patches, double *sims, double *best,
                              uint8_t *keep)
{
    if (!ctx || !imgL || !imgR || nL < 0 || !row_ptr || (nL > 0 && !L))
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    int64_t np = 0;
    if (check_csr(row_ptr, nL, &np) || (np > 0 && !Rc))
        return EBVO_ERR_ARG;
    if (nL == 0)
        return EBVO_OK;
    const size_t nLz = (size_t)nL, npz = (size_t)np;
    if (hc.image(0, imgL, h, w, strideL) || hc.image(1, imgR, h, w, strideR) || hc.grow(s.scratch_b, sizeof(ebvo_edge) * nLz) ||
        hc.grow(s.rc_edges, sizeof(ebvo_edge) * (npz + 1)) || hc.grow(s.row_ptr, sizeof(int32_t) * (nLz + 1)) ||
        hc.grow(s.patches_raw, sizeof(float) * 98 * nLz) || hc.grow(s.patches_norm, sizeof(float) * 98 * nLz) ||
        hc.grow(s.patches_flag, 2 * nLz) || (sims && hc.grow(s.sims, sizeof(double) * 4 * (npz + 1))) ||
        hc.grow(s.best, sizeof(double) * (npz + 1)) || hc.grow(s.keep, npz + 1) || hc.up(s.scratch_b.p, L, sizeof(ebvo_edge) * nLz) ||
        hc.up(s.rc_edges.p, Rc, sizeof(ebvo_edge) * npz) || hc.up(s.row_ptr.p, row_ptr, sizeof(int32_t) * (nLz + 1)))
        return hc.rc;
    int rc;
    if ((rc = match_patches_enqueue(ctx, s, s.im[0].img, h, w, w, (const ebvo_edge *)s.scratch_b.p, nL, nullptr, 0,
                                    (float *)s.patches_raw.p, (float *)s.patches_norm.p, (uint8_t *)s.patches_flag.p)) ||
        (rc = match_ncc_pairs_enqueue(ctx, s, s.im[1].img, h, w, w, (const ebvo_edge *)s.rc_edges.p,
                                      (const int32_t *)s.row_ptr.p, nL, np, (const float *)s.patches_norm.p,
                                      (const uint8_t *)s.patches_flag.p, thr, sims ? (double *)s.sims.p : nullptr,
                                      (double *)s.best.p, (uint8_t *)s.keep.p)))
        return rc;
    hc.down(left_patches, s.patches_raw.p, sizeof(float) * 98 * nLz);
    hc.down(sims, s.sims.p, sizeof(double) * 4 * npz);
    hc.down(best, s.best.p, sizeof(double) * npz);
    hc.down(keep, s.keep.p, npz);
    return hc.finish();
}

extern "C" int ebvo_ncc_patches(ebvo_ctx *ctx, const float *A, const float *B, int n, double *sim)
{
    if (!ctx || n < 0 || (n > 0 && (!A || !B || !sim)))
        return EBVO_ERR_ARG;
    if (n == 0) // (before the slot is taken: an empty list leaves the pair as it is)
        return EBVO_OK;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    const size_t pb = sizeof(float) * 49 * (size_t)n;
    if (hc.grow(s.scratch_b, pb) || hc.grow(s.scratch_c, pb) || hc.grow(s.scratch_d, sizeof(double) * (size_t)n) ||
        hc.up(s.scratch_b.p, A, pb) || hc.up(s.scratch_c.p, B, pb))
        return hc.rc;
    if (int rc = match_ncc_stored_enqueue(ctx, s, (const float *)s.scratch_b.p, (const float *)s.scratch_c.p, n,
                                          (double *)s.scratch_d.p))
        return rc;
    hc.down(sim, s.scratch_d.p, sizeof(double) * (size_t)n);
    return hc.finish();
}

extern "C" int ebvo_ncc_quads(ebvo_ctx *ctx, const float *kfL, const float *kfR, const float *cfL, const float *cfR,
                              int n, double thr, double *sim_left, double *sim_right, uint8_t *keep)
{
    if (!ctx || n < 0 || (n > 0 && (!kfL || !kfR || !cfL || !cfR || !sim_left || !sim_right)))
        return EBVO_ERR_ARG;
    if (n == 0)
        return EBVO_OK;
    // 8 stored-patch NCCs per quad, order of src/Temporal_Matches.cpp:441-450:
    // (first,first) (first,second) (second,first) (second,second), left then right
    std::vector<float> A((size_t)n * 8 * 49), B((size_t)n * 8 * 49);
    for (int k = 0; k < n; ++k)
        for (int m = 0; m < 8; ++m)
        {
            const float *kf = (m < 4 ? kfL : kfR) + (size_t)k * 98 + ((m >> 1) & 1) * 49;
            const float *cf = (m < 4 ? cfL : cfR) + (size_t)k * 98 + (m & 1) * 49;
            memcpy(&A[((size_t)k * 8 + m) * 49], kf, sizeof(float) * 49);
            memcpy(&B[((size_t)k * 8 + m) * 49], cf, sizeof(float) * 49);
        }
    std::vector<double> sv((size_t)n * 8);
    int rc = ebvo_ncc_patches(ctx, A.data(), B.data(), n * 8, sv.data());
    if (rc)
        return rc;
    for (int k = 0; k < n; ++k)
    {
        double sl = sv[(size_t)k * 8], sr = sv[(size_t)k * 8 + 4];
        for (int m = 1; m < 4; ++m)
        {
            if (sl < sv[(size_t)k * 8 + m]) sl = sv[(size_t)k * 8 + m];
            if (sr < sv[(size_t)k * 8 + 4 + m]) sr = sv[(size_t)k * 8 + 4 + m];
        }
        sim_left[k] = sl;
        sim_right[k] = sr;
        if (keep)
            keep[k] = (sl > thr && sr > thr) ? 1 : 0; // :452
    }
    return EBVO_OK;
}

// ------------------------------------------------------------------------------------------
// Device-resident pipeline.  A pair is ENQUEUED without any host synchronisation: every size lives in device
// memory, every launch is sized by a capacity, the last kernel gathers the counts, one async copy brings them to
// pinned host memory.  ebvo_stereo_wait synchronises the slot's stream, and only if the candidate list did not
// fit the pair-indexed buffers does it grow them and re-enqueue the matching half.
extern "C" void ebvo_stereo_default_params(ebvo_stereo_params *p)
{
    if (!p)
        return;
    memset(p, 0, sizeof *p);
    p->epi_thr = EBVO_EPIPOLAR_LINE_DIST_THRESH;
    p->max_disp = EBVO_MAX_DISPARITY;
    p->orient_thr_deg = EBVO_ORIENT_THRESH_DEG;
    p->ncc_thr = EBVO_NCC_THRESH;
    p->stage_mask = EBVO_STAGE_ALL;
}

extern "C" void ebvo_finalize_default_params(ebvo_finalize_params *p)
{
    if (!p)
        return;
    memset(p, 0, sizeof *p);
    p->bnb_ratio = EBVO_BNB_NCC;
    p->ncc_thr = EBVO_NCC_THRESH;
    ebvo_gn_default_params(&p->gn);
    p->use_sift = 0;
    p->sift_thr = EBVO_SIFT_THRESHOLD;
    p->bnb_sift = EBVO_BNB_SIFT;
}

static int get_slot(ebvo_ctx *ctx, int slot, Slot **out)
{
    if (!ctx || slot < 0 || slot >= (int)ctx->slots.size())
        return EBVO_ERR_ARG;
    *out = ctx->slots[(size_t)slot];
    return EBVO_OK;
}

extern "C" int ebvo_stereo_set_slots(ebvo_ctx *ctx, int n_slots)
{
    if (!ctx || n_slots < 1 || n_slots > 64)
        return EBVO_ERR_ARG;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    while ((int)ctx->slots.size() < n_slots)
    {
        Slot *s = nullptr;
        int rc = slot_create(ctx, &s);
        if (rc)
            return rc;
        ctx->slots.push_back(s);
    }
    return EBVO_OK;
}

extern "C" int ebvo_stereo_upload_slot(ebvo_ctx *ctx, int slot, const uint8_t *img_left, const uint8_t *img_right,
                                       int h, int w, ptrdiff_t stride_left, ptrdiff_t stride_right)
{
    Slot *sp;
    int rc;
    // every argument and the slot's state are checked before anything of the slot changes: a refused call leaves the
    // resident pair, its results and the stage-wise tags as they were
    if ((rc = get_slot(ctx, slot, &sp)))
        return rc;
    if (!img_left || !img_right)
        return EBVO_ERR_ARG;
    if ((rc = check_size(ctx, h, w)))
        return rc;
    if (stride_left < w || stride_right < w)
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.in_flight || s.fin_in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    s.have_pair = s.have_run = s.have_refined = s.have_final = false; // results of the previous pair are gone
    s.gt_armed = false; // the ground truth was given for the pair that ran
    s.have_push = false;
    if (slot == 0)
        ctx->sw_tag[0] = ctx->sw_tag[1] = 0; // ... and so are the TOED results of the resident stage-wise calls
    s.tq_n = -1;
    s.tq_final.n = -1;
    s.tq_trail = Slot::TqTrail();
    s.sift_left_valid = false;
    if ((rc = drain_fetch(ctx, s))) // a result copy of the previous pair still reads the buffers / an asynchronous upload writes them
        return rc;
    s.fetch_pending = false;
    s.fetch_what = 0;
    s.undist_pair = ctx->undist_on; // the pair goes to the raw buffers; submit undistorts it into img
    s.toed_strict_override = false;
    s.pull = false;
    if ((rc = upload_image(ctx, s, 0, img_left, h, w, stride_left, s.undist_pair)))
        return rc;
    if ((rc = upload_image(ctx, s, 1, img_right, h, w, stride_right, s.undist_pair)))
        return rc;
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    s.cur_h = h;
    s.cur_w = w;
    s.have_pair = true;
    return EBVO_OK;
}

// The same upload without blocking the calling thread: the two copies go to the context's UPLOAD stream (its own hardware
// queue: they never sit in front of a pair's kernels), an event marks their end, and the slot's next submission makes its
// stream wait for that event -- satisfied long before when the caller uploads a slot a frame ahead of submitting it
// (src/Pipeline.cpp:77-99 reads frame k + 1 while frame k is matched).  Asynchronous only for page-locked sources
// (ebvo_host_register / hipHostMalloc); pageable images are copied into the slot's page-locked staging before the call returns.
extern "C" int ebvo_stereo_upload_async(ebvo_ctx *ctx, int slot, const uint8_t *img_left, const uint8_t *img_right, int h, int w,
                                        ptrdiff_t stride_left, ptrdiff_t stride_right)
{
    Slot *sp;
    int rc;
    // (validated in full before the slot's state changes, as in ebvo_stereo_upload_slot)
    if ((rc = get_slot(ctx, slot, &sp)))
        return rc;
    if (!img_left || !img_right)
        return EBVO_ERR_ARG;
    if ((rc = check_size(ctx, h, w)))
        return rc;
    if (stride_left < w || stride_right < w)
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.in_flight || s.fin_in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    s.have_pair = s.have_run = s.have_refined = s.have_final = false;
    s.gt_armed = false; // the ground truth was given for the pair that ran
    if (slot == 0)
        ctx->sw_tag[0] = ctx->sw_tag[1] = 0;
    s.tq_n = -1;
    s.tq_final.n = -1;
    s.tq_trail = Slot::TqTrail();
    s.sift_left_valid = false;
    s.pull = false;
    if (!ctx->ingest_stream) // (the pull form makes no runtime call at all)
    {
        // pull form: both images entirely in page-locked memory the device can address?  Then the pair's own chain reads them
        // (its first kernel; the pointers go through the slot's mailbox) -- no copy engine, no second stream, no event: nothing
        // that could queue behind another pair's kernels.  Page-locked = inside a range registered with ebvo_host_register.
        const uint8_t *imgs[2] = {img_left, img_right};
        const ptrdiff_t strides[2] = {stride_left, stride_right};
        const uint8_t *dev[2] = {nullptr, nullptr};
        bool pinned = true;
        for (int k = 0; k < 2 && pinned; ++k)
        {
            const size_t span = (size_t)(h - 1) * (size_t)strides[k] + (size_t)w;
            pinned = false;
            for (const ebvo_ctx::HostRange &r : ctx->host_ranges)
                if (imgs[k] >= r.host && imgs[k] + span <= r.host + r.bytes)
                {
                    dev[k] = r.dev + (imgs[k] - r.host);
                    pinned = true;
                    break;
                }
        }
        if (pinned)
        {
            if ((rc = drain_stream_upload(ctx, s)))
                return rc;
            for (int k = 0; k < 2; ++k)
            {
                s.h_mail->src[k] = dev[k];
                s.h_mail->stride[k] = (long long)strides[k];
            }
            s.pull = true;
            ++ctx->pull_uploads;
            s.undist_pair = ctx->undist_on;
            s.toed_strict_override = false;
            s.cur_h = h;
            s.cur_w = w;
            s.have_pair = true;
            return EBVO_OK;
        }
    }
    ++ctx->stream_uploads;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->upload_stream)
        EBVO_HIP(ctx, hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking));
    // ordering on the device, not on the host: result copies of the previous pair (copy stream) still read the edge lists --
    // not the images -- so only a previous asynchronous upload of this slot (same stream: ordered) and the slot's own stream
    // (later stages of the previous pair sample the images) matter
    // The copies below wait ON THE DEVICE for the slot's earlier work, so the runtime cannot read a pageable source while this
    // call runs: it would read it whenever the copy gets its turn -- after the caller has, rightly, freed the images (seen as
    // a GPU memory fault at a host heap address in a later test, once in five full test runs).  Images that are not inside a
    // registered range are therefore copied into the slot's own page-locked staging first (a host memcpy of 2 h w bytes); the
    // previous asynchronous upload of the slot has left the staging when drain_stream_upload returns.
    const uint8_t *src[2] = {img_left, img_right};
    ptrdiff_t sstride[2] = {stride_left, stride_right};
    {
        const size_t npx = (size_t)h * w;
        bool staged = false;
        for (int k = 0; k < 2; ++k)
        {
            const size_t span = (size_t)(h - 1) * (size_t)sstride[k] + (size_t)w;
            bool pinned = false;
            for (const ebvo_ctx::HostRange &r : ctx->host_ranges)
                if (src[k] >= r.host && src[k] + span <= r.host + r.bytes)
                    pinned = true;
            if (pinned)
                continue;
            if (!staged)
            {
                if ((rc = drain_stream_upload(ctx, s)))
                    return rc;
                if (s.h_up_bytes < 2 * npx)
                {
                    if (s.h_up)
                        (void)hipHostFree(s.h_up);
                    s.h_up = nullptr;
                    s.h_up_bytes = 0;
                    if (hipHostMalloc(reinterpret_cast<void **>(&s.h_up), 2 * npx) != hipSuccess)
                    {
                        (void)hipGetLastError();
                        ctx->last_error = "hipHostMalloc failed (staging of ebvo_stereo_upload_async)";
                        return EBVO_ERR_NOMEM;
                    }
                    s.h_up_bytes = 2 * npx;
                }
                staged = true;
            }
            uint8_t *stage = s.h_up + (size_t)k * npx;
            if (sstride[k] == (ptrdiff_t)w)
                memcpy(stage, src[k], npx);
            else
                for (int y = 0; y < h; ++y)
                    memcpy(stage + (size_t)y * w, src[k] + (size_t)y * sstride[k], (size_t)w);
            src[k] = stage;
            sstride[k] = w;
        }
    }
    EBVO_HIP(ctx, hipEventRecord(s.ev_upload, s.own_stream));
    EBVO_HIP(ctx, hipStreamWaitEvent(ctx->upload_stream, s.ev_upload, 0));
    s.undist_pair = ctx->undist_on;
    s.toed_strict_override = false;
    if ((rc = upload_image(ctx, s, 0, src[0], h, w, sstride[0], s.undist_pair, ctx->upload_stream)) ||
        (rc = upload_image(ctx, s, 1, src[1], h, w, sstride[1], s.undist_pair, ctx->upload_stream)))
        return rc;
    EBVO_HIP(ctx, hipEventRecord(s.ev_upload, ctx->upload_stream));
    s.upload_pending = true;
    s.cur_h = h;
    s.cur_w = w;
    s.have_pair = true;
    return EBVO_OK;
}

// Page-locks caller memory (a frame ring, say) so that uploads from it are asynchronous DMA and result copies into it need no
// staging.  Thin wrappers: the host side of the boundary needs no HIP header.
extern "C" int ebvo_host_register(ebvo_ctx *ctx, void *p, size_t bytes)
{
    if (!ctx || !p || !bytes)
        return EBVO_ERR_ARG;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    ebvo_ctx::HostRange r;
    r.host = static_cast<const uint8_t *>(p);
    r.bytes = bytes;
    hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e == hipSuccess)
        r.ours = true;
    else
    {
        // memory that is page-locked already (hipHostMalloc, an earlier registration) is accepted as it is
        (void)hipGetLastError();
        hipPointerAttribute_t a;
        memset(&a, 0, sizeof a);
        if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeHost)
        {
            (void)hipGetLastError();
            return ebvo_fail_hip(ctx, e, "hipHostRegister", __FILE__, __LINE__);
        }
    }
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess || !d)
    {
        (void)hipGetLastError();
        if (r.ours)
            (void)hipHostUnregister(p);
        ctx->last_error = "hipHostGetDevicePointer failed for the registered range";
        return EBVO_ERR_HIP;
    }
    r.dev = static_cast<const uint8_t *>(d);
    ctx->host_ranges.push_back(r);
    return EBVO_OK;
}

// how many ebvo_stereo_upload_async calls took the pull form / the upload stream so far (a frame loop checks that its ring is
// really registered: a pageable source silently takes the slow form)
extern "C" int ebvo_ingest_stats(const ebvo_ctx *ctx, int64_t out[2])
{
    if (!ctx || !out)
        return EBVO_ERR_ARG;
    out[0] = ctx->pull_uploads;
    out[1] = ctx->stream_uploads;
    return EBVO_OK;
}

extern "C" int ebvo_host_unregister(ebvo_ctx *ctx, void *p)
{
    if (!ctx || !p)
        return EBVO_ERR_ARG;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    // a slot whose chain pulls its images from page-locked caller memory must not be submitted again with them: it needs a new
    // upload first (conservative: the library does not know which registration a mailbox points into)
    for (Slot *sl : ctx->slots)
        if (sl->pull)
        {
            if (sl->in_flight)
                EBVO_HIP(ctx, hipEventSynchronize(sl->ev_done));
            sl->pull = false;
            if (!sl->in_flight)
                sl->have_pair = false;
        }
    bool ours = false, found = false;
    for (size_t k = 0; k < ctx->host_ranges.size(); ++k)
        if (ctx->host_ranges[k].host == p)
        {
            ours = ctx->host_ranges[k].ours;
            found = true;
            ctx->host_ranges.erase(ctx->host_ranges.begin() + (ptrdiff_t)k);
            break;
        }
    if (!found)
        return EBVO_ERR_ARG;
    if (ours)
        EBVO_HIP(ctx, hipHostUnregister(p));
    return EBVO_OK;
}

extern "C" int ebvo_stereo_upload(ebvo_ctx *ctx, const uint8_t *img_left, const uint8_t *img_right, int h, int w,
                                  ptrdiff_t stride_left, ptrdiff_t stride_right)
{
    return ebvo_stereo_upload_slot(ctx, 0, img_left, img_right, h, w, stride_left, stride_right);
}

// capacity-sized buffers of the pipeline
static int ensure_pipeline_buffers(ebvo_ctx *ctx, Slot &s, int64_t cap_pairs)
{
    const size_t ce = (size_t)ctx->cap_edges;
    int rc;
    if ((rc = ebvo_grow(ctx, s, s.lines, sizeof(double) * 3 * ce)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.patches_raw, sizeof(float) * 98 * ce)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.patches_norm, sizeof(float) * 98 * ce)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.patches_flag, 2 * ce)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.patches_norm_r, match_right_bank_bytes(ctx->cap_edges))))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.sincos, sizeof(double) * 2 * ce)))
        return rc;
    const size_t cp = (size_t)cap_pairs;
    if ((rc = ebvo_grow(ctx, s, s.col_idx, sizeof(int32_t) * cp)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.pair_left, sizeof(int32_t) * cp)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.sims, sizeof(double) * 4 * cp)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.best, sizeof(double) * cp)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.keep, cp)))
        return rc;
    s.cap_pairs = cap_pairs;
    s.pipe_cap = cap_pairs;
    return EBVO_OK;
}

// lines -> candidates<count> -> [row offsets + staged rows || right patch bank] -> long-row redo -> LDS-tiled NCC -> result
// record; no host synchronisation
static int enqueue_matching(ebvo_ctx *ctx, Slot &s, int toed_mode = -1)
{
    const ebvo_stereo_params &p = s.params;
    const int h = s.cur_h, w = s.cur_w, ce = ctx->cap_edges;
    const int32_t *d_nL = s.im[0].counts + 1, *d_nR = s.im[1].counts + 1;
    int rc;
    // lines, boxes, sin / cos and row-pair images in one launch (round 4: four launches of ~5 us each before)
    const bool prep = !ctx->no_prep;
    const int stop = ctx->stop_stage; // (developer key 16: the counts of the last whole run stay in the pair's record)
    if (stop && stop <= 7)
        return EBVO_OK;
    if (prep ? (rc = match_prep_enqueue(ctx, s, h, w, ce))
             : (rc = match_lines_enqueue(ctx, s, s.d_F, s.im[0].edges, 0, d_nL, ce, (double *)s.lines.p)))
        return rc;
    if (stop == 8)
        return EBVO_OK;
    if ((rc = match_candidates_enqueue(ctx, s, s.im[0].edges, 0, d_nL, s.im[1].edges, 0, d_nR, ce,
                                       (const double *)s.lines.p, p.epi_thr, p.max_disp, p.orient_thr_deg, p.stage_mask,
                                       true, prep)))
        return rc;
    if (stop == 9)
        return EBVO_OK;
    if ((rc = match_ncc_resident_enqueue(ctx, s, h, w, ce, p.ncc_thr, 0, !(p.reserved & EBVO_PAIR_NO_SIMS), prep, &p)))
        return rc;
    if (stop)
        return EBVO_OK;
    // a hybrid TOED run reports candidate lists that did not fit through the result record (bit 1, value 2, of `overflow`)
    if ((rc = match_pair_result_enqueue(ctx, s, (toed_mode < 0 ? ctx->toed_mode : toed_mode) == EBVO_TOED_HYBRID ? ce : 0)))
        return rc;
    return EBVO_OK; // the caller records s.ev_done behind it (outside a stream capture)
}

// undistortion (if the pair was uploaded raw) + TOED of both images + matching: every launch of one pair
// EBVO_PAIR_PUSH: the compact results of a pair written by the device into page-locked host memory, as the last kernel of the
// pair's chain (same arrays as ebvo_stereo_fetch_compact_begin; the sizes are read on the device).  Coalesced 16-byte stores
// over PCIe; the kernel holds a handful of CUs while the lanes' other pairs compute.
namespace
{
// where the eight arrays lie in a packed result block, from the ACTUAL counts (the device reads them where the host computes
// the same offsets after ebvo_stereo_wait): xyL, xyR, thL, thR, row_ptr, col_idx, best, keep bits; 256-byte aligned
struct PackLayout
{
    size_t off[8], total;
};
__host__ __device__ inline PackLayout pack_layout(size_t nL, size_t nR, size_t np, bool theta)
{
    const size_t sizes[8] = {16 * nL, 16 * nR, theta ? 8 * nL : 0, theta ? 8 * nR : 0, 4 * (nL + 1), 4 * np, 8 * np, 8 * ((np + 63) >> 6)};
    PackLayout l;
    size_t t = 0;
    for (int k = 0; k < 8; ++k)
    {
        l.off[k] = t;
        t += (sizes[k] + 255) & ~(size_t)255;
    }
    l.total = t;
    return l;
}

__global__ __launch_bounds__(256) void push_results_kernel(const ebvo_edge *__restrict__ L, const ebvo_edge *__restrict__ R,
                                                           const int32_t *__restrict__ nLp, const int32_t *__restrict__ nRp, int cap_edges,
                                                           const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                           const double *__restrict__ best, const uint8_t *__restrict__ keep,
                                                           int64_t cap_pairs, char *__restrict__ base, int theta)
{
    const int nL = min(*nLp, cap_edges), nR = min(*nRp, cap_edges);
    int64_t np = nL > 0 ? (int64_t)row_ptr[nL] : 0;
    np = np < cap_pairs ? np : cap_pairs;
    const PackLayout lay = pack_layout((size_t)nL, (size_t)nR, (size_t)np, theta != 0);
    double2 *xyL = (double2 *)(base + lay.off[0]), *xyR = (double2 *)(base + lay.off[1]);
    double *thL = theta ? (double *)(base + lay.off[2]) : nullptr, *thR = theta ? (double *)(base + lay.off[3]) : nullptr;
    int32_t *o_rp = (int32_t *)(base + lay.off[4]), *o_ci = (int32_t *)(base + lay.off[5]);
    double *o_best = (double *)(base + lay.off[6]);
    uint32_t *o_bits = (uint32_t *)(base + lay.off[7]);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < nL; i += stride)
    {
        const ebvo_edge e = L[i];
        xyL[i] = make_double2(e.x, e.y);
        if (thL)
            thL[i] = e.theta;
    }
    for (int64_t i = t0; i < nR; i += stride)
    {
        const ebvo_edge e = R[i];
        xyR[i] = make_double2(e.x, e.y);
        if (thR)
            thR[i] = e.theta;
    }
    for (int64_t i = t0; i <= nL; i += stride)
        o_rp[i] = row_ptr[i];
    // four CSR entries / two scores per thread: 16-byte stores
    const int64_t n4 = np >> 2;
    for (int64_t i = t0; i < n4; i += stride)
        reinterpret_cast<int4 *>(o_ci)[i] = reinterpret_cast<const int4 *>(col_idx)[i];
    for (int64_t i = (n4 << 2) + t0; i < np; i += stride)
        o_ci[i] = col_idx[i];
    const int64_t n2 = np >> 1;
    for (int64_t i = t0; i < n2; i += stride)
        reinterpret_cast<double2 *>(o_best)[i] = reinterpret_cast<const double2 *>(best)[i];
    if ((np & 1) && t0 == 0)
        o_best[np - 1] = best[np - 1];
    const int64_t groups = (np + 63) >> 6, wave = t0 >> 6, waves = stride >> 6;
    const int lane = threadIdx.x & 63;
    for (int64_t g = wave; g < groups; g += waves)
    {
        const int64_t k = (g << 6) + lane;
        const unsigned long long m = __ballot(k < np && keep[k] != 0);
        if (lane == 0)
        {
            o_bits[2 * g] = (uint32_t)m;
            o_bits[2 * g + 1] = (uint32_t)(m >> 32);
        }
    }
}
} // namespace

// (re)sizes the destination of the chain's pack kernel for the capacities the chain is enqueued with: the slot's page-locked
// arena (EBVO_PAIR_PUSH) or its device staging (EBVO_PAIR_PACK).  A re-allocation bumps buf_gen (the address is an argument of
// a captured launch).
static int ensure_push_arena(ebvo_ctx *ctx, Slot &s)
{
    const bool theta = s.params.reserved & EBVO_PAIR_PUSH_THETA;
    const size_t total = pack_layout((size_t)ctx->cap_edges, (size_t)ctx->cap_edges, (size_t)s.cap_pairs, theta).total;
    if (s.params.reserved & EBVO_PAIR_PUSH)
    {
        if (total > s.push_bytes)
        {
            if (s.h_push)
                (void)hipHostFree(s.h_push);
            s.h_push = s.d_push = nullptr;
            s.push_bytes = 0;
            if (hipHostMalloc(&s.h_push, total) != hipSuccess)
            {
                (void)hipGetLastError();
                ctx->last_error = "hipHostMalloc failed (page-locked result arena of EBVO_PAIR_PUSH)";
                return EBVO_ERR_NOMEM;
            }
            EBVO_HIP(ctx, hipHostGetDevicePointer(&s.d_push, s.h_push, 0));
            s.push_bytes = total;
            ++s.buf_gen;
        }
        return EBVO_OK;
    }
    if (total > s.fetch_pack.bytes && s.fetch_pending) // copies out of the old staging must be over before it is replaced
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_rebind));
    return ebvo_grow(ctx, s, s.fetch_pack, total);
}

// the images of a pair, read by the GPU from the caller's page-locked memory (ebvo_stereo_upload_async): 16 bytes per thread
namespace
{
__global__ __launch_bounds__(256) void pull_images_kernel(const Slot::PullMail *__restrict__ mail, uint8_t *__restrict__ d0,
                                                          uint8_t *__restrict__ d1, int h, int w)
{
    const uint8_t *__restrict__ src = mail->src[blockIdx.y];
    const long long stride = mail->stride[blockIdx.y];
    uint8_t *__restrict__ dst = blockIdx.y ? d1 : d0;
    const int per_row = (w + 15) >> 4; // 16-byte pieces per row (the last one may be short)
    const long long pieces = (long long)h * per_row;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < pieces; t += (long long)gridDim.x * blockDim.x)
    {
        const int y = (int)(t / per_row), c = (int)(t - (long long)y * per_row) << 4;
        const uint8_t *sp = src + (long long)y * stride + c;
        uint8_t *dp = dst + (size_t)y * w + c;
        if (c + 16 <= w)
        {
            uint4 v;
            __builtin_memcpy(&v, sp, 16);
            __builtin_memcpy(dp, &v, 16);
        }
        else
            for (int k = 0; c + k < w; ++k)
                dp[k] = sp[k];
    }
}
} // namespace

static int enqueue_push(ebvo_ctx *ctx, Slot &s)
{
    if (!(s.params.reserved & (EBVO_PAIR_PUSH | EBVO_PAIR_PACK)))
        return EBVO_OK;
    char *base = static_cast<char *>((s.params.reserved & EBVO_PAIR_PUSH) ? s.d_push : s.fetch_pack.p);
    hipLaunchKernelGGL(push_results_kernel, dim3(64), dim3(256), 0, s.stream, (const ebvo_edge *)s.im[0].edges,
                       (const ebvo_edge *)s.im[1].edges, (const int32_t *)(s.im[0].counts + 1), (const int32_t *)(s.im[1].counts + 1),
                       ctx->cap_edges, (const int32_t *)s.row_ptr.p, (const int32_t *)s.col_idx.p, (const double *)s.best.p,
                       (const uint8_t *)s.keep.p, s.cap_pairs, base, (s.params.reserved & EBVO_PAIR_PUSH_THETA) ? 1 : 0);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}

static int enqueue_pair_chain(ebvo_ctx *ctx, Slot &s)
{
    int rc;
    if (s.pull)
    {
        hipLaunchKernelGGL(pull_images_kernel, dim3(64, 2), dim3(256), 0, s.stream, (const Slot::PullMail *)s.d_mail,
                           s.undist_pair ? s.im[0].raw : s.im[0].img, s.undist_pair ? s.im[1].raw : s.im[1].img, s.cur_h, s.cur_w);
        EBVO_HIP(ctx, hipGetLastError());
    }
    if (s.undist_pair) // cv::undistort of both raw images (src/Pipeline.cpp:78-79); TOED runs on the result (:93, :97)
    {
        const ebvo_undistort_params &u = ctx->undist;
        if ((rc = refine_undistort_enqueue(ctx, s, s.im[0].raw, s.cur_w, s.cur_h, s.cur_w, u.K_left, u.dist_left, u.n_dist,
                                           s.im[0].undist_xs, s.im[0].img, s.cur_w)) ||
            (rc = refine_undistort_enqueue(ctx, s, s.im[1].raw, s.cur_w, s.cur_h, s.cur_w, u.K_right, u.dist_right, u.n_dist,
                                           s.im[1].undist_xs, s.im[1].img, s.cur_w)))
            return rc;
    }
    // (no subpix_edge_pts_final in the resident pipeline: nothing downstream reads it, 8 MB of scattered stores per pair)
    const int mode = s.toed_strict_override ? EBVO_TOED_STRICT : -1;
    if ((rc = toed_enqueue(ctx, s, 2, s.cur_h, s.cur_w, nullptr, nullptr, nullptr, mode, false)))
        return rc;
    if ((rc = enqueue_matching(ctx, s, mode)))
        return rc;
    return enqueue_push(ctx, s);
}

static void pair_graph_drop(Slot &s)
{
    if (s.pair_graph)
        (void)hipGraphExecDestroy(s.pair_graph);
    s.pair_graph = nullptr;
}

// The chain of one pair is 16 launches whose arguments depend only on PairGraphKey and on the slot's buffers (the sizes
// of everything live on the device): the second submission with an unchanged key captures it, later ones launch the graph
// (measured, tools/ubench/graph_launch.hip: 7-20 us of host time for a 30-kernel chain against 86 us of direct launches,
// and ~2 us instead of ~2.9 us between dependent kernels on the device).  Anything unusual -- profiling markers, a key
// that changed, a capture that fails -- takes the direct path; `first` reports that to the caller for its statistics.
static int submit_pair_chain(ebvo_ctx *ctx, Slot &s)
{
    PairGraphKey key;
    memset(&key, 0, sizeof key);
    key.h = s.cur_h;
    key.w = s.cur_w;
    key.toed_mode = s.toed_strict_override ? EBVO_TOED_STRICT : ctx->toed_mode;
    key.undist = (s.undist_pair ? 1 : 0) | (s.pull ? 2 : 0);
    key.cap_pairs = s.cap_pairs;
    key.gen = ctx->graph_gen + (s.buf_gen << 20);
    key.epi_thr = s.params.epi_thr;
    key.max_disp = s.params.max_disp;
    key.orient_thr_deg = s.params.orient_thr_deg;
    key.ncc_thr = s.params.ncc_thr;
    key.stage_mask = s.params.stage_mask;
    key.flags = s.params.reserved;
    const bool same = memcmp(&key, &s.pair_key, sizeof key) == 0;
    const bool eligible = ctx->use_graphs && !s.pair_graph_off && !ctx->prof && !s.prof_now;
    if (!same)
    {
        pair_graph_drop(s);
        s.pair_key = key;
        s.pair_key_warm = false;
    }
    int rc;
    if (eligible && s.pair_graph)
    {
        EBVO_HIP(ctx, hipGraphLaunch(s.pair_graph, s.stream));
        ++ctx->graph_launches;
        return EBVO_OK;
    }
    if (eligible && s.pair_key_warm)
    {
        // capture: thread-local mode, so that other host threads keep using their own streams meanwhile
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamBeginCapture(s.stream, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess)
        {
            const uint64_t gen_before = s.buf_gen;
            rc = enqueue_pair_chain(ctx, s);
            e = hipStreamEndCapture(s.stream, &g); // always: the stream must leave capture mode
            if (rc == EBVO_OK && e == hipSuccess && g && s.buf_gen == gen_before)
                e = hipGraphInstantiate(&s.pair_graph, g, nullptr, nullptr, 0);
            else if (e == hipSuccess)
                e = hipErrorUnknown;
            if (g)
                (void)hipGraphDestroy(g);
        }
        if (e == hipSuccess && s.pair_graph)
        {
            EBVO_HIP(ctx, hipGraphLaunch(s.pair_graph, s.stream));
            ++ctx->graph_launches;
            return EBVO_OK;
        }
        (void)hipGetLastError();
        pair_graph_drop(s);
        s.pair_graph_off = true; // and fall through to the direct launches
    }
    if ((rc = enqueue_pair_chain(ctx, s)))
        return rc;
    if (ctx->graph_gen + (s.buf_gen << 20) == s.pair_key.gen)
        s.pair_key_warm = true; // nothing was (re)allocated on the way: the next submission may capture
    return EBVO_OK;
}

extern "C" int ebvo_stereo_submit(ebvo_ctx *ctx, int slot, const ebvo_stereo_params *p)
{
    Slot *sp;
    if (!p || (p->stage_mask & ~EBVO_STAGE_ALL) || p->stage_mask == 0 || (p->reserved & ~(EBVO_PAIR_NO_SIMS | EBVO_PAIR_PUSH | EBVO_PAIR_PUSH_THETA | EBVO_PAIR_PACK)) ||
        !stereo_thresholds_ok(p->epi_thr, p->max_disp, p->orient_thr_deg, p->ncc_thr) ||
        ((p->reserved & EBVO_PAIR_PUSH) && (p->reserved & EBVO_PAIR_PACK)) || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_pair || s.in_flight || s.fin_in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    s.have_run = s.have_refined = s.have_final = false;
    s.gt_armed = false; // the ground truth was given for the pair that ran
    const bool fetch_was_pending = s.fetch_pending;
    s.fetch_pending = false; // stream order (or the event below): the kernels run after any copy still enqueued
    s.fetch_what = 0;
    s.params = *p;
    s.have_sims = !(p->reserved & EBVO_PAIR_NO_SIMS);
    s.prof_now = ctx->prof && (ctx->prof_submits++ % ctx->prof_every == 0);
    // lanes in use: none up to three slots (one stream each), never as many lanes as slots (a lane must be able to hold
    // a queued pair behind the running one: four slots on four streams is the 2500 pairs/s dip)
    const int n_lanes = ((int)ctx->slots.size() >= 4 && ctx->lanes > 0)
                            ? (ctx->lanes < (int)ctx->slots.size() - 1 ? ctx->lanes : (int)ctx->slots.size() - 1)
                            : 0;
    if (n_lanes > 0)
    {
        // Four or more pairs in flight: their KERNELS are dealt round-robin to a few streams of the context ("lanes")
        // instead of one stream per slot.  Measured (tools/gpu_streams_sweep.py, tools/gpu_lanes_sweep.py, KITTI pair): one
        // stream per slot gives 2010 / 2540 / 2800 pairs/s for 1 / 2 / 3 slots and then DROPS (2500 at 4 slots, 2700 at 5;
        // GPU_MAX_HW_QUEUES and stream priorities do not change that); three lanes give 2850-2880 for 4 ... 12 slots, four
        // lanes 2920-2945 for 5 ... 16 slots, five and six lanes less.  Everything else a slot does (uploads, fetch copies,
        // the later stages) stays on its own stream: ebvo_stereo_wait hands the slot back to it once the host has seen
        // the pair complete, and the only work a slot can leave pending there -- the copies of ebvo_stereo_fetch_begin --
        // carries an event.
        while ((int)ctx->lane_streams.size() < n_lanes)
        {
            hipStream_t st = nullptr;
            EBVO_HIP(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            ctx->lane_streams.push_back(st);
        }
        hipStream_t lane = ctx->lane_streams[ctx->submit_seq++ % (uint64_t)n_lanes];
        s.stream = lane;
    }
    if (fetch_was_pending) // result copies of the previous pair (on the copy stream) still read the buffers
        EBVO_HIP(ctx, hipStreamWaitEvent(s.stream, s.ev_rebind, 0));
    if (s.upload_pending) // the pair's images arrive on the upload stream (ebvo_stereo_upload_async)
        EBVO_HIP(ctx, hipStreamWaitEvent(s.stream, s.ev_upload, 0));
    s.upload_pending = false;
    struct Unbind // a submission that fails leaves the slot on its own stream
    {
        Slot &s;
        ~Unbind()
        {
            if (!s.in_flight)
                s.stream = s.own_stream;
        }
    } unbind{s};
    {
        int64_t want = s.pipe_cap > 0 ? s.pipe_cap : 8 * (int64_t)ctx->cap_edges;
        if (want < 4096)
            want = 4096;
        if ((rc = ensure_pipeline_buffers(ctx, s, want)))
            return rc;
    }
    s.have_push = s.have_pack = false;
    if ((s.params.reserved & (EBVO_PAIR_PUSH | EBVO_PAIR_PACK)) && (rc = ensure_push_arena(ctx, s)))
        return rc;
    // the fundamental matrix goes up only when it differs from what the device holds (a sequence has ONE; the copy of 72 bytes
    // from pageable memory is a blit kernel of ~5 us at the head of the chain otherwise)
    if (!s.F_dev_valid || memcmp(s.F_dev, s.params.F21, sizeof s.F_dev) != 0)
    {
        EBVO_HIP(ctx, hipMemcpyAsync(s.d_F, s.params.F21, sizeof(double) * 9, hipMemcpyHostToDevice, s.stream));
        memcpy(s.F_dev, s.params.F21, sizeof s.F_dev);
        s.F_dev_valid = true;
    }
    if ((rc = submit_pair_chain(ctx, s)))
        return rc;
    EBVO_HIP(ctx, hipEventRecord(s.ev_done, s.stream));
    s.in_flight = true;
    return EBVO_OK;
}

extern "C" int ebvo_stereo_wait(ebvo_ctx *ctx, int slot, ebvo_stereo_counts *counts)
{
    Slot *sp;
    if (!counts || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = EBVO_OK;
    struct Restore
    {
        Slot &s;
        ~Restore()
        {
            s.prof_now = true; // host-buffer calls on this slot are always bracketed
            if (!s.in_flight)
                s.stream = s.own_stream; // the pair ran on a lane (ebvo_stereo_submit); the host has seen it complete
        }
    } restore{s};
    bool have_result = false;
    const int max_attempts = ctx->wait_attempts > 0 ? ctx->wait_attempts : 4;
    for (int attempt = 0; attempt < max_attempts; ++attempt)
    {
        // the event behind this pair's last kernel, not the stream: a lane may already hold the next pair of another slot
        hipError_t e = hipEventSynchronize(s.ev_done);
        if (e != hipSuccess)
        {
            s.in_flight = false;
            return ebvo_fail_hip(ctx, e, "hipEventSynchronize", __FILE__, __LINE__);
        }
        const PairResult r = *s.h_result;
        if (r.overflow & 2)
        {
            // the hybrid screen flagged more candidates than fit (toed_compact_phase_kernel): the whole pair again, strict
            ++ctx->toed_fallbacks;
            s.toed_strict_override = true; // remembered until the next upload: these images go strict at once from now on
            if ((rc = toed_enqueue(ctx, s, 2, s.cur_h, s.cur_w, nullptr, nullptr, nullptr, EBVO_TOED_STRICT, false)) ||
                (rc = enqueue_matching(ctx, s, EBVO_TOED_STRICT)) || (rc = enqueue_push(ctx, s)))
            {
                s.in_flight = false;
                return rc;
            }
            EBVO_HIP(ctx, hipEventRecord(s.ev_done, s.stream));
            --attempt; // not a regrowth: the fallback does not use up one of the attempts (it happens at most once per wait)
            continue;
        }
        if (r.n_total_left > ctx->cap_edges || r.n_total_right > ctx->cap_edges)
        {
            s.in_flight = false;
            ctx->last_error = "internal edge capacity exceeded";
            return EBVO_ERR_CAPACITY;
        }
        if (!r.overflow && !(ctx->force_overflow > 0 && ctx->force_overflow-- > 0))
        {
            s.result = r;
            have_result = true;
            break;
        }
        if (r.n_pairs > 0x7fffffffll)
        {
            s.in_flight = false;
            ctx->last_error = "candidate list exceeds 2^31-1 pairs";
            return EBVO_ERR_CAPACITY;
        }
        // more candidates than the buffers hold: grow them and redo the matching half (TOED results are intact)
        int64_t want = r.n_pairs + r.n_pairs / 4 + 1024;
        if ((rc = ensure_pipeline_buffers(ctx, s, want)) ||
            ((s.params.reserved & (EBVO_PAIR_PUSH | EBVO_PAIR_PACK)) && (rc = ensure_push_arena(ctx, s))) ||
            (rc = enqueue_matching(ctx, s)) || (rc = enqueue_push(ctx, s)))
        {
            s.in_flight = false;
            return rc;
        }
        EBVO_HIP(ctx, hipEventRecord(s.ev_done, s.stream));
    }
    if (!have_result)
    {
        // every attempt reported an overflow: the last re-enqueued matching half is still running; never publish a
        // stale s.result
        (void)hipEventSynchronize(s.ev_done);
        s.in_flight = false;
        ctx->last_error = "candidate buffers still too small after regrowing (ebvo_stereo_wait gave up)";
        return EBVO_ERR_CAPACITY;
    }
    s.in_flight = false;
    s.im[0].n_kept = s.result.n_left;
    s.im[0].n_total = s.result.n_total_left;
    s.im[1].n_kept = s.result.n_right;
    s.im[1].n_total = s.result.n_total_right;
    counts->n_left = s.result.n_left;
    counts->n_right = s.result.n_right;
    counts->n_total_left = s.result.n_total_left;
    counts->n_total_right = s.result.n_total_right;
    counts->n_pairs = s.result.n_pairs;
    counts->n_matches = s.result.n_matches;
    s.have_run = true;
    s.have_push = (s.params.reserved & EBVO_PAIR_PUSH) != 0;
    s.have_pack = (s.params.reserved & EBVO_PAIR_PACK) != 0;
    return EBVO_OK;
}

static void fill_compact_view(ebvo_stereo_compact_view *view, const char *b, const PackLayout &lay, const PairResult &r, bool theta)
{
    memset(view, 0, sizeof *view);
    view->n_left = r.n_left;
    view->n_right = r.n_right;
    view->n_pairs = r.n_pairs;
    view->n_matches = r.n_matches;
    view->left_xy = reinterpret_cast<const double *>(b + lay.off[0]);
    view->right_xy = reinterpret_cast<const double *>(b + lay.off[1]);
    if (theta)
    {
        view->left_theta = reinterpret_cast<const double *>(b + lay.off[2]);
        view->right_theta = reinterpret_cast<const double *>(b + lay.off[3]);
    }
    view->row_ptr = reinterpret_cast<const int32_t *>(b + lay.off[4]);
    view->col_idx = reinterpret_cast<const int32_t *>(b + lay.off[5]);
    view->best = reinterpret_cast<const double *>(b + lay.off[6]);
    view->keep_bits = reinterpret_cast<const uint32_t *>(b + lay.off[7]);
}

// the compact results a pair submitted with EBVO_PAIR_PUSH left in the slot's page-locked arena: valid from the pair's
// ebvo_stereo_wait until the slot's next submission
extern "C" int ebvo_stereo_pushed_view(ebvo_ctx *ctx, int slot, ebvo_stereo_compact_view *view)
{
    Slot *sp;
    if (!view || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.in_flight || !s.have_push || !s.h_push)
        return EBVO_ERR_STATE;
    const char *b = static_cast<const char *>(s.h_push);
    const bool theta = s.params.reserved & EBVO_PAIR_PUSH_THETA;
    const PackLayout lay = pack_layout((size_t)s.result.n_left, (size_t)s.result.n_right, (size_t)s.result.n_pairs, theta);
    fill_compact_view(view, b, lay, s.result, theta);
    return EBVO_OK;
}

extern "C" int ebvo_stereo_run(ebvo_ctx *ctx, const ebvo_stereo_params *p, ebvo_stereo_counts *counts)
{
    if (!ctx || !p || !counts)
        return EBVO_ERR_ARG;
    int rc = ebvo_stereo_submit(ctx, 0, p);
    if (rc)
        return rc;
    return ebvo_stereo_wait(ctx, 0, counts);
}

// ------------------------------------------------------------------------------------------
// Resident stage-wise path.  main_VO calls the stages one after the other (src/Pipeline.cpp:24-29, :93-97,
// src/Stereo_Matches.cpp:1374-1427) and hands every stage the vectors the previous one returned.  The calls below keep
// what a stage produced on the device (slot 0's two image workspaces: edges, counts) under a TAG, take tags instead of
// edge arrays, and return their results as pointers into page-locked memory of the context: nothing that the device
// already holds is uploaded again, no result passes through pageable memory.  A tag dies when its workspace gets another
// edge list: the next ebvo_toed_resident on it, ebvo_toed / ebvo_toed_pair, a pair uploaded into slot 0.  The other
// host-buffer entry points (SIFT, Best-Nearly-Best, refinement, ... -- what get_Stereo_Edge_Pairs calls between the stages)
// use slot 0's scratch buffers and image planes only and leave the tags valid.  A caller that cannot present valid tags
// gets EBVO_ERR_STATE and uses the host-buffer calls.
static int pinned_grow(ebvo_ctx *ctx, PinnedBuf &b, size_t bytes)
{
    if (bytes <= b.bytes)
        return EBVO_OK;
    if (b.p)
        EBVO_HIP(ctx, hipHostFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipHostMalloc(&b.p, want);
    if (e != hipSuccess)
    {
        b.p = nullptr;
        ebvo_fail_hip(ctx, e, "hipHostMalloc (stage-wise result arena)", __FILE__, __LINE__);
        return e == hipErrorOutOfMemory ? EBVO_ERR_NOMEM : EBVO_ERR_HIP;
    }
    b.bytes = want;
    return EBVO_OK;
}

// Host-to-device copy of caller memory through the context's page-locked staging (`off` bytes into sw_up, which the caller
// has sized).  The caller's buffers are ordinary pageable memory (a cv::Mat, a std::vector) that it frees or reuses right
// after the call: copying out of them directly makes the runtime lock their pages for the transfer, and unmapping locked
// pages later stalls the next submission (measured: ~1 ms on the first call of the next frame).
static int upload_staged(ebvo_ctx *ctx, Slot &s, void *d_dst, const void *src, size_t bytes, size_t off)
{
    if (!bytes)
        return EBVO_OK;
    char *stage = (char *)ctx->sw_up.p + off;
    memcpy(stage, src, bytes);
    EBVO_HIP(ctx, hipMemcpyAsync(d_dst, stage, bytes, hipMemcpyHostToDevice, s.stream));
    return EBVO_OK;
}
static int upload_image_staged(ebvo_ctx *ctx, Slot &s, int k, const uint8_t *img, int h, int w, ptrdiff_t stride, size_t off)
{
    if (stride < w)
        return EBVO_ERR_ARG;
    uint8_t *stage = (uint8_t *)ctx->sw_up.p + off;
    if (stride == (ptrdiff_t)w)
        memcpy(stage, img, (size_t)w * h);
    else
        for (int y = 0; y < h; ++y)
            memcpy(stage + (size_t)y * w, img + (size_t)y * stride, (size_t)w);
    EBVO_HIP(ctx, hipMemcpyAsync(s.im[k].img, stage, (size_t)w * h, hipMemcpyHostToDevice, s.stream));
    return EBVO_OK;
}

extern "C" int ebvo_toed_resident(ebvo_ctx *ctx, int which, const uint8_t *img, int h, int w, ptrdiff_t stride,
                                  int want_all4, ebvo_toed_view *view)
{
    if (!ctx || !img || !view || which < 0 || which > 1)
        return EBVO_ERR_ARG;
    memset(view, 0, sizeof *view);
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    Slot *sp;
    if ((rc = check_size(ctx, h, w)) || (rc = host_slot(ctx, &sp)))
        return rc;
    Slot &s = *sp;
    if (ctx->sw_h != h || ctx->sw_w != w) // the two workspaces of a slot hold images of ONE size
        ctx->sw_tag[0] = ctx->sw_tag[1] = 0;
    ctx->sw_h = h;
    ctx->sw_w = w;
    ctx->sw_tag[which] = 0;
    static const bool trace = getenv("EBVO_TRACE_STAGEWISE") != nullptr;
    auto tnow = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tt[6] = {0};
    if (trace)
        tt[0] = tnow();
    if ((rc = pinned_grow(ctx, ctx->sw_up, (size_t)h * w + 64)) || (rc = upload_image_staged(ctx, s, which, img, h, w, stride, 0)))
        return rc;
    if (trace)
    {
        tt[1] = tnow();
        (void)hipStreamSynchronize(s.stream);
        tt[2] = tnow();
    }
    float ms_c = 0, ms_n = 0;
    {
        // TOED of ONE image, in place in workspace `which`: the enqueue walks workspaces 0 .. n - 1, so the two are swapped
        // around it (plain pointer records; the kernels hold their own copies of the pointers)
        struct Swap
        {
            Slot &s;
            bool on;
            Swap(Slot &s_, bool on_) : s(s_), on(on_)
            {
                if (on)
                    std::swap(s.im[0], s.im[1]);
            }
            ~Swap()
            {
                if (on)
                    std::swap(s.im[0], s.im[1]);
            }
        } swap_ws(s, which == 1);
        if ((rc = toed_sync(ctx, s, 1, h, w, &ms_c, &ms_n)))
            return rc;
    }
    if (trace)
        tt[3] = tnow();
    const ImageWS &ws = s.im[which];
    view->n_kept = ws.n_kept;
    view->n_total = ws.n_total;
    view->t_conv = ms_c * 1e-3;
    view->t_nms = ms_n * 1e-3;
    if (ws.n_total > ctx->cap_edges)
    {
        ctx->last_error = "internal edge capacity exceeded";
        return EBVO_ERR_CAPACITY;
    }
    const size_t eb = round_up64(sizeof(ebvo_edge) * (size_t)ws.n_kept), ab = want_all4 ? sizeof(double) * 4 * (size_t)ws.n_total : 0;
    PinnedBuf &pb = ctx->sw_toed[which];
    if ((rc = pinned_grow(ctx, pb, eb + ab + 64)))
        return rc;
    if (ws.n_kept)
        EBVO_HIP(ctx, hipMemcpyAsync(pb.p, ws.edges, sizeof(ebvo_edge) * (size_t)ws.n_kept, hipMemcpyDeviceToHost, s.stream));
    if (ab)
        EBVO_HIP(ctx, hipMemcpyAsync((char *)pb.p + eb, ws.all4, ab, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    if (trace)
    {
        tt[4] = tnow();
        fprintf(stderr, "[ebvo] toed_resident(%d): upload call %.3f, upload done %.3f, toed + counts %.3f, result copies %.3f ms (device %.3f)\n",
                which, (tt[1] - tt[0]) * 1e3, (tt[2] - tt[1]) * 1e3, (tt[3] - tt[2]) * 1e3, (tt[4] - tt[3]) * 1e3, ms_c + ms_n);
    }
    view->edges = (const ebvo_edge *)pb.p;
    view->all4 = want_all4 ? (const double *)((char *)pb.p + eb) : nullptr;
    view->tag = ctx->sw_tag[which] = ++ctx->sw_seq;
    return EBVO_OK;
}

// which workspace holds `tag` (0 / 1), -1 if neither does
static int resident_ws(const ebvo_ctx *ctx, uint64_t tag)
{
    if (tag != 0 && ctx->sw_tag[0] == tag)
        return 0;
    if (tag != 0 && ctx->sw_tag[1] == tag)
        return 1;
    return -1;
}

extern "C" int ebvo_epi_candidates_resident(ebvo_ctx *ctx, uint64_t tag_left, uint64_t tag_right, const double *lines,
                                            double epi_thr, double max_disp, double orient_thr_deg, int stage_mask,
                                            int want_orient_flags, ebvo_candidates_view *view)
{
    if (!ctx || !view || (stage_mask & ~EBVO_STAGE_ALL) || stage_mask == 0 ||
        !stereo_thresholds_ok(epi_thr, max_disp, orient_thr_deg, 0.0))
        return EBVO_ERR_ARG;
    memset(view, 0, sizeof *view);
    const int iL = resident_ws(ctx, tag_left), iR = resident_ws(ctx, tag_right);
    if (iL < 0 || iR < 0 || iL == iR)
    {
        ctx->last_error = "the edge lists named by the tags are no longer resident";
        return EBVO_ERR_STATE;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    Slot *sp;
    if ((rc = host_slot(ctx, &sp)))
        return rc;
    Slot &s = *sp;
    const int nL = s.im[iL].n_kept, nR = s.im[iR].n_kept;
    if (nL > 0 && !lines)
        return EBVO_ERR_ARG;
    const size_t rb = round_up64(sizeof(int32_t) * ((size_t)nL + 1));
    if ((rc = pinned_grow(ctx, ctx->sw_cand, rb + 64)))
        return rc;
    view->row_ptr = (const int32_t *)ctx->sw_cand.p;
    if (nL == 0 || nR == 0)
    {
        memset(ctx->sw_cand.p, 0, rb);
        if (want_orient_flags)
            view->row_ptr_final = view->row_ptr; // all zeros
        return EBVO_OK;
    }
    if ((rc = ebvo_grow(ctx, s, s.lines, sizeof(double) * 3 * (size_t)nL)))
        return rc;
    if ((rc = pinned_grow(ctx, ctx->sw_up, sizeof(double) * 3 * (size_t)nL + 64)) ||
        (rc = upload_staged(ctx, s, s.lines.p, lines, sizeof(double) * 3 * (size_t)nL, 0)))
        return rc;
    const ebvo_edge *dL = s.im[iL].edges, *dR = s.im[iR].edges;
    s.cap_pairs = 0;
    if ((rc = match_candidates_enqueue(ctx, s, dL, nL, nullptr, dR, nR, nullptr, 0, (const double *)s.lines.p, epi_thr,
                                       max_disp, orient_thr_deg, stage_mask, false)))
    {
        (void)hipStreamSynchronize(s.stream); // the copy out of the caller's `lines` may still be in flight
        return rc;
    }
    unsigned long long *h_total_p = reinterpret_cast<unsigned long long *>(s.h_result);
    {
        hipError_t e1 = hipMemcpyAsync(h_total_p, s.d_total, sizeof(*h_total_p), hipMemcpyDeviceToHost, s.stream);
        hipError_t e2 = e1 == hipSuccess ? hipMemcpyAsync(ctx->sw_cand.p, s.row_ptr.p, sizeof(int32_t) * ((size_t)nL + 1),
                                                          hipMemcpyDeviceToHost, s.stream)
                                         : hipSuccess;
        hipError_t e3 = hipStreamSynchronize(s.stream);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
            return ebvo_fail_hip(ctx, e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3), "candidate total read-back",
                                 __FILE__, __LINE__);
    }
    const unsigned long long h_total = *h_total_p;
    if (h_total > 0x7fffffffull)
    {
        ctx->last_error = "candidate list exceeds 2^31-1 pairs";
        return EBVO_ERR_CAPACITY;
    }
    const int64_t np = (int64_t)h_total;
    view->n_pairs = np;
    if (np == 0)
    {
        if (want_orient_flags)
            view->row_ptr_final = view->row_ptr; // all zeros
        return EBVO_OK;
    }
    // arena: row_ptr | col_idx | flags | row_ptr_final | col_idx_final (the final list is a sub-list: np bounds it)
    const bool staged = want_orient_flags != 0;
    const size_t cb = round_up64(sizeof(int32_t) * (size_t)np), fb = staged ? round_up64((size_t)np) : 0;
    const size_t rb2 = staged ? rb : 0, cb2 = staged ? cb : 0;
    {
        // growing the arena moves it: the row offsets already copied are kept
        PinnedBuf &pb = ctx->sw_cand;
        const size_t need = rb + cb + fb + rb2 + cb2 + 64;
        if (pb.bytes < need)
        {
            PinnedBuf fresh;
            if ((rc = pinned_grow(ctx, fresh, need)))
                return rc;
            memcpy(fresh.p, pb.p, rb);
            (void)hipHostFree(pb.p);
            pb = fresh;
        }
        view->row_ptr = (const int32_t *)pb.p;
    }
    if ((rc = ebvo_grow(ctx, s, s.col_idx, sizeof(int32_t) * (size_t)np)))
        return rc;
    s.cap_pairs = np;
    char *base = (char *)ctx->sw_cand.p;
    unsigned long long *h_final_p = h_total_p + 1; // second word of the slot's pinned record
    static_assert(sizeof(PairResult) >= 2 * sizeof(unsigned long long), "pinned record too small for two totals");
    rc = [&]() -> int {
        int r;
        if ((r = match_candidates_fill_enqueue(ctx, s, dL, nL, nullptr, dR, nR, nullptr, 0, (const double *)s.lines.p, epi_thr,
                                               max_disp, orient_thr_deg, stage_mask)))
            return r;
        if (staged)
        {
            if ((r = ebvo_grow(ctx, s, s.keep, (size_t)np)) ||
                (r = match_orient_flags_enqueue(ctx, s, dL, nL, dR, (const int32_t *)s.row_ptr.p, (const int32_t *)s.col_idx.p,
                                                np, orient_thr_deg, (uint8_t *)s.keep.p)))
                return r;
        }
        EBVO_HIP(ctx, hipMemcpyAsync(base + rb, s.col_idx.p, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, s.stream));
        if (staged)
        {
            EBVO_HIP(ctx, hipMemcpyAsync(base + rb + cb, s.keep.p, (size_t)np, hipMemcpyDeviceToHost, s.stream));
            // the list the flags select = the search under all three predicates (stream order: the copies above have read
            // row_ptr / col_idx before these kernels overwrite them); it fits the buffers of the longer list
            if ((r = match_candidates_enqueue(ctx, s, dL, nL, nullptr, dR, nR, nullptr, 0, (const double *)s.lines.p, epi_thr,
                                              max_disp, orient_thr_deg, stage_mask | EBVO_STAGE_ORIENTATION, false)) ||
                (r = match_candidates_fill_enqueue(ctx, s, dL, nL, nullptr, dR, nR, nullptr, 0, (const double *)s.lines.p, epi_thr,
                                                   max_disp, orient_thr_deg, stage_mask | EBVO_STAGE_ORIENTATION)))
                return r;
            EBVO_HIP(ctx, hipMemcpyAsync(h_final_p, s.d_total, sizeof(*h_final_p), hipMemcpyDeviceToHost, s.stream));
            EBVO_HIP(ctx, hipMemcpyAsync(base + rb + cb + fb, s.row_ptr.p, sizeof(int32_t) * ((size_t)nL + 1),
                                         hipMemcpyDeviceToHost, s.stream));
        }
        return EBVO_OK;
    }();
    hipError_t es = hipStreamSynchronize(s.stream);
    int64_t nf = 0;
    if (!rc && es == hipSuccess && staged)
    {
        nf = (int64_t)*h_final_p;
        if (nf > np) // cannot happen: a sub-list
        {
            ctx->last_error = "internal: the orientation-filtered list is longer than the list it filters";
            rc = EBVO_ERR_HIP;
        }
        else if (nf > 0)
        {
            hipError_t e = hipMemcpyAsync(base + rb + cb + fb + rb2, s.col_idx.p, sizeof(int32_t) * (size_t)nf, hipMemcpyDeviceToHost,
                                          s.stream);
            es = hipStreamSynchronize(s.stream);
            if (e != hipSuccess)
                es = e;
        }
    }
    s.cap_pairs = 0; // the pipeline re-establishes its own capacity
    if (rc)
        return rc;
    EBVO_HIP(ctx, es);
    view->col_idx = (const int32_t *)(base + rb);
    view->orient_ok = staged ? (const uint8_t *)(base + rb + cb) : nullptr;
    if (staged)
    {
        view->row_ptr_final = (const int32_t *)(base + rb + cb + fb);
        view->col_idx_final = (const int32_t *)(base + rb + cb + fb + rb2);
        view->n_final = nf;
    }
    return EBVO_OK;
}

extern "C" int ebvo_ncc_pairs_resident(ebvo_ctx *ctx, uint64_t tag_left, uint64_t tag_right, const uint8_t *imgL,
                                       const uint8_t *imgR, int h, int w, ptrdiff_t strideL, ptrdiff_t strideR,
                                       const int32_t *row_ptr, const int32_t *col_idx, double thr, int want,
                                       ebvo_ncc_view *view)
{
    if (!ctx || !view || !imgL || !imgR || !row_ptr || (want & ~(EBVO_NCC_WANT_LEFT_PATCHES | EBVO_NCC_WANT_SIMS)))
        return EBVO_ERR_ARG;
    memset(view, 0, sizeof *view);
    const int iL = resident_ws(ctx, tag_left), iR = resident_ws(ctx, tag_right);
    if (iL < 0 || iR < 0 || iL == iR)
    {
        ctx->last_error = "the edge lists named by the tags are no longer resident";
        return EBVO_ERR_STATE;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    Slot *sp;
    if ((rc = check_size(ctx, h, w)) || (rc = host_slot(ctx, &sp)))
        return rc;
    Slot &s = *sp;
    if (h != ctx->sw_h || w != ctx->sw_w)
    {
        ctx->last_error = "image size differs from the size the resident edges were detected on";
        return EBVO_ERR_ARG;
    }
    const int nL = s.im[iL].n_kept, nR = s.im[iR].n_kept;
    if (row_ptr[0] != 0)
        return EBVO_ERR_ARG;
    const int64_t np = nL > 0 ? row_ptr[nL] : 0;
    if (np < 0 || (np > 0 && !col_idx))
        return EBVO_ERR_ARG;
    if (nL == 0)
        return EBVO_OK;
    // the lists go through page-locked staging and are validated on the way: the kernels index the right patch bank with
    // col_idx and walk the pair arrays with row_ptr
    const size_t rb = round_up64(sizeof(int32_t) * ((size_t)nL + 1)), cb = round_up64(sizeof(int32_t) * (size_t)np);
    const size_t ib = round_up64((size_t)h * w);
    if ((rc = pinned_grow(ctx, ctx->sw_up, rb + cb + 2 * ib + 64)))
        return rc;
    int32_t *h_rp = (int32_t *)ctx->sw_up.p, *h_ci = (int32_t *)((char *)ctx->sw_up.p + rb);
    {
        int32_t prev = 0, bad = 0;
        for (int i = 0; i <= nL; ++i)
        {
            const int32_t v = row_ptr[i];
            bad |= (v < prev);
            prev = v;
            h_rp[i] = v;
        }
        uint32_t over = 0;
        for (int64_t k = 0; k < np; ++k)
        {
            const int32_t v = col_idx[k];
            over |= ((uint32_t)v >= (uint32_t)nR);
            h_ci[k] = v;
        }
        if (bad || over)
        {
            ctx->last_error = bad ? "row_ptr is not non-decreasing" : "col_idx holds an index outside the resident right edge list";
            return EBVO_ERR_ARG;
        }
    }
    int64_t want_cap = s.pipe_cap > np ? s.pipe_cap : np + np / 4 + 1024;
    if (want_cap < 4096)
        want_cap = 4096;
    if ((rc = ensure_pipeline_buffers(ctx, s, want_cap)))
        return rc;
    if ((rc = ebvo_grow(ctx, s, s.row_ptr, sizeof(int32_t) * ((size_t)ctx->cap_edges + 1))))
        return rc;
    const size_t lb = (want & EBVO_NCC_WANT_LEFT_PATCHES) ? round_up64(sizeof(float) * 98 * (size_t)nL) : 0;
    const size_t sb = (want & EBVO_NCC_WANT_SIMS) ? round_up64(sizeof(double) * 4 * (size_t)np) : 0;
    const size_t bb = round_up64(sizeof(double) * (size_t)np), kb = round_up64((size_t)np);
    if ((rc = pinned_grow(ctx, ctx->sw_ncc, lb + sb + bb + kb + 64)))
        return rc;
    // the images the NCC samples are the RAW ones the caller passes (src/Stereo_Matches.cpp:562-563); they replace the
    // images in the workspaces, the edges stay
    if ((rc = upload_image_staged(ctx, s, iL, imgL, h, w, strideL, rb + cb)) ||
        (rc = upload_image_staged(ctx, s, iR, imgR, h, w, strideR, rb + cb + ib)))
    {
        (void)hipStreamSynchronize(s.stream);
        return rc;
    }
    bool patches_on_copy_stream = false;
    rc = [&]() -> int {
        int r;
        EBVO_HIP(ctx, hipMemcpyAsync(s.row_ptr.p, h_rp, sizeof(int32_t) * ((size_t)nL + 1), hipMemcpyHostToDevice, s.stream));
        if (np)
            EBVO_HIP(ctx, hipMemcpyAsync(s.col_idx.p, h_ci, sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice, s.stream));
        if (lb && (r = match_patches_enqueue(ctx, s, s.im[iL].img, h, w, w, s.im[iL].edges, nL, nullptr, 0,
                                             (float *)s.patches_raw.p, (float *)s.patches_norm.p, (uint8_t *)s.patches_flag.p)))
            return r;
        char *base = (char *)ctx->sw_ncc.p;
        if (lb)
        {
            // the left patches (the largest result: 392 bytes per left edge) travel on the copy stream while the pairs are scored
            if (!ctx->copy_stream)
                EBVO_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
            EBVO_HIP(ctx, hipEventRecord(s.ev_done, s.stream));
            EBVO_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, s.ev_done, 0));
            EBVO_HIP(ctx, hipMemcpyAsync(base, s.patches_raw.p, sizeof(float) * 98 * (size_t)nL, hipMemcpyDeviceToHost,
                                         ctx->copy_stream));
            patches_on_copy_stream = true;
        }
        if (np)
        {
            if ((r = match_ncc_resident_enqueue(ctx, s, h, w, ctx->cap_edges, thr, iL)))
                return r;
            if (sb)
                EBVO_HIP(ctx, hipMemcpyAsync(base + lb, s.sims.p, sizeof(double) * 4 * (size_t)np, hipMemcpyDeviceToHost, s.stream));
            EBVO_HIP(ctx, hipMemcpyAsync(base + lb + sb, s.best.p, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, s.stream));
            EBVO_HIP(ctx, hipMemcpyAsync(base + lb + sb + bb, s.keep.p, (size_t)np, hipMemcpyDeviceToHost, s.stream));
        }
        return EBVO_OK;
    }();
    const hipError_t es = hipStreamSynchronize(s.stream);
    const hipError_t ec = patches_on_copy_stream ? hipStreamSynchronize(ctx->copy_stream) : hipSuccess;
    if (rc)
        return rc;
    EBVO_HIP(ctx, es);
    EBVO_HIP(ctx, ec);
    char *base = (char *)ctx->sw_ncc.p;
    view->n_left = nL;
    view->n_pairs = np;
    view->left_patches = lb ? (const float *)base : nullptr;
    view->sims = sb ? (const double *)(base + lb) : nullptr;
    view->best = np ? (const double *)(base + lb + sb) : nullptr;
    view->keep = np ? (const uint8_t *)(base + lb + sb + bb) : nullptr;
    return EBVO_OK;
}

extern "C" int ebvo_gn_refine_temporal(ebvo_ctx *ctx, const uint8_t *imgKF, const uint8_t *imgCF, int h, int w,
                                       ptrdiff_t strideKF, ptrdiff_t strideCF, const ebvo_edge *kf, const ebvo_edge *cf,
                                       const double *init_disp, int n, const ebvo_gn_params *params, double *disp,
                                       double *score, uint8_t *validity, int32_t *iters)
{
    if (!ctx || !imgKF || !imgCF || n < 0 || !params || params->max_iter < 1 || !(params->tol >= 0) ||
        !(params->huber_delta > 0))
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (n == 0)
        return EBVO_OK;
    if (!kf || !cf || !init_disp || !disp || !score || !validity || !iters)
        return EBVO_ERR_ARG;
    const size_t nz = (size_t)n;
    if (hc.image(0, imgKF, h, w, strideKF) || hc.image(1, imgCF, h, w, strideCF) || hc.grow(s.scratch_b, sizeof(ebvo_edge) * nz) ||
        hc.grow(s.scratch_c, sizeof(ebvo_edge) * nz) || hc.grow(s.gn_xy, sizeof(double) * 2 * nz) ||
        hc.grow(s.gn_out, sizeof(double) * 3 * nz) || hc.grow(s.gn_valid, nz) || hc.grow(s.gn_iters, sizeof(int32_t) * nz) ||
        hc.up(s.scratch_b.p, kf, sizeof(ebvo_edge) * nz) || hc.up(s.scratch_c.p, cf, sizeof(ebvo_edge) * nz) ||
        hc.up(s.gn_xy.p, init_disp, sizeof(double) * 2 * nz))
        return hc.rc;
    double *out = (double *)s.gn_out.p;
    // (the refinement packs the current-frame image itself: intensity + Sobel gradients per bilinear cell)
    if (int rc = refine_gn_temporal_enqueue(ctx, s, s.im[0].img, s.im[1].img, nullptr, h, w,
                                            (const ebvo_edge *)s.scratch_b.p, (const ebvo_edge *)s.scratch_c.p,
                                            (const double *)s.gn_xy.p, n, params->max_iter, params->tol, params->huber_delta,
                                            out, out + 2 * nz, (uint8_t *)s.gn_valid.p, (int32_t *)s.gn_iters.p))
        return rc;
    hc.down(disp, out, sizeof(double) * 2 * nz);
    hc.down(score, out + 2 * nz, sizeof(double) * nz);
    hc.down(validity, s.gn_valid.p, nz);
    hc.down(iters, s.gn_iters.p, sizeof(int32_t) * nz);
    return hc.finish();
}

// ---- stage glue on CSR candidate lists -------------------------------------------------------------------------
static int row_select(ebvo_ctx *ctx, const int32_t *row_ptr, int nL, const double *scores, double thr, int mode,
                      int32_t *new_count, int32_t *order)
{
    int64_t np = 0;
    if (!ctx || check_csr(row_ptr, nL, &np) || (nL > 0 && !new_count) || (np > 0 && (!scores || !order)))
        return EBVO_ERR_ARG;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (nL == 0)
        return EBVO_OK;
    const size_t npz = (size_t)np, nLz = (size_t)nL;
    if (hc.grow(s.row_ptr, sizeof(int32_t) * (nLz + 1)) || hc.grow(s.best, sizeof(double) * (npz + 1)) ||
        hc.grow(s.cand_cnt, sizeof(int32_t) * (nLz + 1)) || hc.grow(s.pair_left, sizeof(int32_t) * (npz + 1)) ||
        hc.up(s.row_ptr.p, row_ptr, sizeof(int32_t) * (nLz + 1)) || hc.up(s.best.p, scores, sizeof(double) * npz))
        return hc.rc;
    const int32_t *d_rp = (const int32_t *)s.row_ptr.p;
    int32_t *d_cnt = (int32_t *)s.cand_cnt.p, *d_order = (int32_t *)s.pair_left.p;
    if (int rc = mode == 2 ? glue_keep_best_enqueue(ctx, s, d_rp, nL, (const double *)s.best.p, d_cnt, d_order)
                           : glue_bnb_enqueue(ctx, s, d_rp, nL, (const double *)s.best.p, thr, mode, d_cnt, d_order))
        return rc;
    hc.down(new_count, d_cnt, sizeof(int32_t) * nLz);
    hc.down(order, d_order, sizeof(int32_t) * npz);
    return hc.finish();
}

extern "C" int ebvo_bnb_test(ebvo_ctx *ctx, const int32_t *row_ptr, int nL, const double *scores, double ratio_thr,
                             int higher_is_better, int32_t *new_count, int32_t *order)
{
    return row_select(ctx, row_ptr, nL, scores, ratio_thr, higher_is_better ? 1 : 0, new_count, order);
}

extern "C" int ebvo_keep_best(ebvo_ctx *ctx, const int32_t *row_ptr, int nL, const double *scores, int32_t *new_count,
                              int32_t *order)
{
    return row_select(ctx, row_ptr, nL, scores, 0.0, 2, new_count, order);
}

extern "C" int ebvo_epipolar_shift(ebvo_ctx *ctx, const ebvo_edge *cand, const double *lines, const int32_t *row_ptr, int nL,
                                   ebvo_edge *shifted)
{
    int64_t np = 0;
    if (!ctx || check_csr(row_ptr, nL, &np) || (np > 0 && (!cand || !lines || !shifted)))
        return EBVO_ERR_ARG;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (np == 0)
        return EBVO_OK;
    const size_t npz = (size_t)np, nLz = (size_t)nL;
    if (hc.grow(s.row_ptr, sizeof(int32_t) * (nLz + 1)) || hc.grow(s.lines, sizeof(double) * 3 * nLz) ||
        hc.grow(s.rc_edges, sizeof(ebvo_edge) * npz) || hc.grow(s.scratch_c, sizeof(ebvo_edge) * npz) ||
        hc.grow(s.pair_left, sizeof(int32_t) * npz) || hc.up(s.row_ptr.p, row_ptr, sizeof(int32_t) * (nLz + 1)) ||
        hc.up(s.lines.p, lines, sizeof(double) * 3 * nLz) || hc.up(s.rc_edges.p, cand, sizeof(ebvo_edge) * npz))
        return hc.rc;
    int rc;
    if ((rc = match_expand_rows_enqueue(ctx, s, (const int32_t *)s.row_ptr.p, nL, np, (int32_t *)s.pair_left.p)) ||
        (rc = glue_shift_enqueue(ctx, s, (const ebvo_edge *)s.rc_edges.p, (const double *)s.lines.p,
                                 (const int32_t *)s.pair_left.p, np, (ebvo_edge *)s.scratch_c.p)))
        return rc;
    hc.down(shifted, s.scratch_c.p, sizeof(ebvo_edge) * npz);
    return hc.finish();
}

extern "C" int ebvo_cluster_rows(ebvo_ctx *ctx, const ebvo_edge *cand, const int32_t *row_ptr, int nL, int by_orientation,
                                 int skip_single, int32_t *new_count, ebvo_edge *centres, int32_t *cluster_of)
{
    int64_t np = 0;
    if (!ctx || check_csr(row_ptr, nL, &np) || (nL > 0 && !new_count) || (np > 0 && (!cand || !centres || !cluster_of)))
        return EBVO_ERR_ARG;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (nL == 0)
        return EBVO_OK;
    const size_t npz = (size_t)np, nLz = (size_t)nL;
    if (hc.grow(s.row_ptr, sizeof(int32_t) * (nLz + 1)) || hc.grow(s.cand_cnt, sizeof(int32_t) * (nLz + 1)) ||
        hc.grow(s.rc_edges, sizeof(ebvo_edge) * (npz + 1)) || hc.grow(s.scratch_c, sizeof(ebvo_edge) * (npz + 1)) ||
        hc.grow(s.pair_left, sizeof(int32_t) * (npz + 1)) || hc.up(s.row_ptr.p, row_ptr, sizeof(int32_t) * (nLz + 1)) ||
        hc.up(s.rc_edges.p, cand, sizeof(ebvo_edge) * npz))
        return hc.rc;
    if (int rc = glue_cluster_enqueue(ctx, s, (const ebvo_edge *)s.rc_edges.p, (const int32_t *)s.row_ptr.p, nL, by_orientation,
                                      skip_single, (int32_t *)s.cand_cnt.p, (ebvo_edge *)s.scratch_c.p, (int32_t *)s.pair_left.p))
        return rc;
    hc.down(new_count, s.cand_cnt.p, sizeof(int32_t) * nLz);
    hc.down(centres, s.scratch_c.p, sizeof(ebvo_edge) * npz);
    hc.down(cluster_of, s.pair_left.p, sizeof(int32_t) * npz);
    return hc.finish();
}

extern "C" int ebvo_finalize_pairs(ebvo_ctx *ctx, const ebvo_stereo_calib *calib, const ebvo_edge *left,
                                   const ebvo_edge *right, int n, double *out16)
{
    if (!ctx || !calib || n < 0 || (n > 0 && (!left || !right || !out16)))
        return EBVO_ERR_ARG;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (n == 0)
        return EBVO_OK;
    const size_t nz = (size_t)n;
    if (hc.grow(s.scratch_b, sizeof(ebvo_edge) * nz) || hc.grow(s.scratch_c, sizeof(ebvo_edge) * nz) ||
        hc.grow(s.gn_out, sizeof(double) * 16 * nz) || hc.up(s.scratch_b.p, left, sizeof(ebvo_edge) * nz) ||
        hc.up(s.scratch_c.p, right, sizeof(ebvo_edge) * nz))
        return hc.rc;
    if (int rc = refine_finalize_pairs_enqueue(ctx, s, calib->K_left, calib->K_right, calib->R21, calib->T21,
                                               (const ebvo_edge *)s.scratch_b.p, (const ebvo_edge *)s.scratch_c.p, n,
                                               (double *)s.gn_out.p))
        return rc;
    hc.down(out16, s.gn_out.p, sizeof(double) * 16 * nz);
    return hc.finish();
}

// ---- photometric refinement of the kept matches of a resident pair ---------------------------------------------
extern "C" int ebvo_stereo_refine(ebvo_ctx *ctx, int slot, const ebvo_gn_params *params)
{
    Slot *sp;
    if (!params || params->max_iter < 1 || !(params->tol >= 0) || !(params->huber_delta > 0) || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_run || s.in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc_f = drain_fetch(ctx, s))
        return rc_f;
    const int64_t np = s.result.n_pairs;
    s.have_refined = false;
    if (np == 0)
    {
        s.have_refined = true;
        return EBVO_OK;
    }
    const int h = s.cur_h, w = s.cur_w;
    const size_t npz = (size_t)np;
    int rc;
    if ((rc = ebvo_grow(ctx, s, s.gn_out, sizeof(double) * 5 * npz)) || (rc = ebvo_grow(ctx, s, s.gn_valid, npz)) ||
        (rc = ebvo_grow(ctx, s, s.gn_iters, sizeof(int32_t) * npz)))
        return rc;
    double *out = (double *)s.gn_out.p;
    // the pipeline's own device arrays: left / right TOED edges, epipolar lines, NCC keep flags; the pair -> left edge
    // expansion of the CSR is formed here (the matching kernels themselves work per tile of rows)
    if ((rc = ebvo_grow(ctx, s, s.pair_left, sizeof(int32_t) * npz)) ||
        (rc = match_expand_rows_enqueue(ctx, s, (const int32_t *)s.row_ptr.p, s.result.n_left, np, (int32_t *)s.pair_left.p)) ||
        (rc = refine_gn_stereo_enqueue(ctx, s, s.im[0].img, s.im[1].img, nullptr, h, w, s.im[0].edges, s.result.n_left,
                                       (const double *)s.lines.p, (const int32_t *)s.pair_left.p, nullptr, s.im[1].edges,
                                       (const int32_t *)s.col_idx.p, (const uint8_t *)s.keep.p, np, params->max_iter,
                                       params->tol, params->huber_delta, out, out + npz, out + 2 * npz,
                                       (uint8_t *)s.gn_valid.p, (int32_t *)s.gn_iters.p, out + 3 * npz)))
        return rc;
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    s.have_refined = true;
    return EBVO_OK;
}

extern "C" int ebvo_stereo_fetch_refined(ebvo_ctx *ctx, int slot, double *alpha, double *score, double *confidence,
                                         uint8_t *validity, int32_t *iters, double *refined_xy)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_refined || s.in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npz = (size_t)s.result.n_pairs;
    if (!npz)
        return EBVO_OK;
    const double *out = (const double *)s.gn_out.p;
    hipStream_t st = s.stream;
    if (alpha)
        EBVO_HIP(ctx, hipMemcpyAsync(alpha, out, sizeof(double) * npz, hipMemcpyDeviceToHost, st));
    if (score)
        EBVO_HIP(ctx, hipMemcpyAsync(score, out + npz, sizeof(double) * npz, hipMemcpyDeviceToHost, st));
    if (confidence)
        EBVO_HIP(ctx, hipMemcpyAsync(confidence, out + 2 * npz, sizeof(double) * npz, hipMemcpyDeviceToHost, st));
    if (refined_xy)
        EBVO_HIP(ctx, hipMemcpyAsync(refined_xy, out + 3 * npz, sizeof(double) * 2 * npz, hipMemcpyDeviceToHost, st));
    if (validity)
        EBVO_HIP(ctx, hipMemcpyAsync(validity, s.gn_valid.p, npz, hipMemcpyDeviceToHost, st));
    if (iters)
        EBVO_HIP(ctx, hipMemcpyAsync(iters, s.gn_iters.p, sizeof(int32_t) * npz, hipMemcpyDeviceToHost, st));
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    return EBVO_OK;
}

// ---- the stages after the NCC pass, on the resident pair: [SIFT filter ->] BNB -> shift -> refine -> cluster -> NCC -> best
// Every stage is the kernel behind the corresponding host-buffer entry point; only the CSR bookkeeping between them is
// new (glue_kernels.hip).  The chain is ENQUEUED: a stage's survivor count stays on the device (the last entry of the
// scanned row offsets), the next stage's kernels are launched for the upper bound (the pair count of the run: every stage
// only shrinks the lists) and read the count there.  The six stage totals travel to page-locked memory in one copy behind
// the last kernel; ebvo_stereo_finalize_wait is the only host synchronisation.  No candidate data leaves HBM.
static int read_i32(ebvo_ctx *ctx, Slot &s, const int32_t *d, int32_t *h)
{
    EBVO_HIP(ctx, hipMemcpyAsync(h, d, sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    return EBVO_OK;
}

// developer key 23 holds for the launches ebvo_stereo_finalize_submit enqueues only: the helpers this chain shares with the
// pair chain, the temporal chain and the host-buffer calls read Slot::fin_blocks, which is zero outside this scope
struct FinalizeGridScope
{
    Slot &s;
    FinalizeGridScope(const ebvo_ctx *ctx, Slot &slot) : s(slot) { s.fin_blocks = ctx->finalize_blocks; }
    ~FinalizeGridScope() { s.fin_blocks = 0; }
};

static int finalize_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_finalize_params *p, const ebvo_stereo_calib *calib)
{
    const int nL = s.result.n_left, h = s.cur_h, w = s.cur_w;
    const int64_t n0 = s.result.n_pairs;
    const size_t nz = (size_t)n0, nLz = (size_t)nL + 1;
    int rc;
    // carve the work buffers: everything is bounded by the pair count of the run (each stage only shrinks the lists)
    if ((rc = ebvo_grow(ctx, s, s.fin_i32, sizeof(int32_t) * (4 * nLz + 4 * nz))) ||
        (rc = ebvo_grow(ctx, s, s.fin_edges, sizeof(ebvo_edge) * (3 * nz + 2 * nLz))) ||
        (rc = ebvo_grow(ctx, s, s.fin_f64, sizeof(double) * (5 * nz + nLz) + 16 * nz)) ||
        (rc = ebvo_grow(ctx, s, s.fin_u8, nz)) || (rc = ebvo_grow(ctx, s, s.fin_out, sizeof(double) * 16 * nLz)) ||
        (rc = ebvo_grow(ctx, s, s.gn_xy, sizeof(double) * 2 * nz)) || (rc = ebvo_grow(ctx, s, s.gn_out, sizeof(double) * 5 * nz)) ||
        (rc = ebvo_grow(ctx, s, s.gn_valid, nz)) || (rc = ebvo_grow(ctx, s, s.gn_iters, sizeof(int32_t) * nz)))
        return rc;
    // (the final lists keep their places: ebvo_stereo_fetch_final and the temporal stage read final_left, fin_l / fin_r and
    // fin_score at these offsets)
    int32_t *cnt = (int32_t *)s.fin_i32.p, *rpA = cnt + nLz, *rpB = rpA + nLz, *final_left = rpB + nLz;
    int32_t *order = final_left + nLz, *left_of = order + nz, *cluster_of = left_of + nz, *ncc_left = cluster_of + nz;
    ebvo_edge *candA = (ebvo_edge *)s.fin_edges.p, *candB = candA + nz, *candC = candB + nz, *fin_l = candC + nz,
              *fin_r = fin_l + nLz;
    double *scoreA = (double *)s.fin_f64.p, *scoreB = scoreA + nz, *best2 = scoreB + nz, *fin_score = best2 + nz;
    double *confA = fin_score + nLz, *confB = confA + nz; // SIFT distances carried through the Best-Nearly-Best tests
    void *sincos2 = confB + nz; // n0 double2
    uint8_t *keep2 = (uint8_t *)s.fin_u8.p;
    const int32_t *rp0 = (const int32_t *)s.row_ptr.p;
    hipStream_t st = s.stream;
    int32_t *tot = s.d_fin_tot;
    EBVO_HIP(ctx, hipMemsetAsync(tot, 0, sizeof(int32_t) * 8, st));
    auto scan_counts = [&](int32_t *rp_out, int which) -> int {
        // exclusive scan of cnt[0 .. nL) with the total at rp_out[nL]; the scan also stores it as stage total `which`
        // (no memset of a trailing zero, no copy of the total: two launches less per stage)
        return ebvo_device_scan(ctx, s, cnt, rp_out, nL, nullptr, 1, nL + 1, tot + which);
    };
    enum { T_SIFT = 0, T_NCC, T_BNB, T_CLUSTERS, T_NCC2, T_FINAL };
    const uint8_t *keep1 = (const uint8_t *)s.keep.p;
    const double *conf0 = nullptr; // SIFT distance per pair of the run (refine_confidences, :757)
    // Evaluate_Stereo_Edge_Correspondences after a stage (:1419-1521) when, and only when, the slot is armed
    // (ebvo_stereo_set_gt): the (n, tp) of every row of the stage's list and its integer totals; reads the lists only
    const bool gt_on = s.gt_armed;
    auto gt_eval = [&](int stage, const int32_t *rp, const ebvo_edge *cand, const uint8_t *flags) -> int {
        if (!gt_on)
            return EBVO_OK;
        return gt_rows_enqueue(ctx, s, rp, cand, cand ? nullptr : (const int32_t *)s.col_idx.p, s.im[1].edges, flags,
                               (const double *)s.gt_geom.p, (const uint8_t *)s.gt_flags.p + s.gt_nL, nL, s.gt_params.tp_dist,
                               (int32_t *)s.gt_rows.p + (size_t)stage * 2 * nL, (unsigned long long *)s.gt_tot.p + (size_t)stage * 8);
    };
    if (p->use_sift)
    {
        // 0. augment_Edge_Data (:1410) + apply_SIFT_filtering (:1414): descriptors of every left and right TOED edge on the
        // undistorted images (each right edge once, not once per left edge that lists it), the smallest of the four
        // distances per candidate pair, dist < thr.  NCC scores do not depend on which pairs survive, so the SIFT filter
        // applied to the NCC-scored pairs of the run selects the reference's SIFT-then-NCC survivors.
        const int nR = s.result.n_right;
        const size_t npx = (size_t)h * w;
        if ((rc = ebvo_grow(ctx, s, s.sift_img, sizeof(float) * 3 * npx)) ||
            (rc = ebvo_grow(ctx, s, s.sift_desc, 256 * ((size_t)nL + (size_t)nR))) ||
            (rc = ebvo_grow(ctx, s, s.sift_dist, sizeof(double) * nz + 2 * nz)) ||
            (rc = ebvo_grow(ctx, s, s.pair_left, sizeof(int32_t) * nz)) ||
            (rc = ebvo_grow(ctx, s, s.sift_used, sizeof(int32_t) * (4 + (size_t)nL + (size_t)nR) + (size_t)nR)))
            return rc;
        float *tmp = (float *)s.sift_img.p, *base = tmp + npx, *base1 = base + npx; // (both octave bases: one descriptor launch)
        uint8_t *dL = (uint8_t *)s.sift_desc.p, *dR = dL + 256 * (size_t)nL;
        double *dist = (double *)s.sift_dist.p;
        uint8_t *ok = (uint8_t *)(dist + nz), *both = ok + nz;
        // Only an edge that appears in a candidate pair has its descriptor read (by the distances below; the temporal stage
        // reuses those of the final mates' left edges): on the EuRoC-shaped pair that is 45 % of the edges of either image
        // (1.2 candidates per left edge; KITTI-shaped: 97 %), and the descriptors are the dearest kernel of this chain.
        int32_t *used_cnt = (int32_t *)s.sift_used.p, *usedL = used_cnt + 4, *usedR = usedL + nL;
        uint8_t *used_flags = (uint8_t *)(usedR + nR);
        if ((rc = sift_used_edges_enqueue(ctx, s, rp0, nL, (const int32_t *)s.col_idx.p, n0, nR, used_cnt, usedL, usedR, used_flags)) ||
            (rc = sift_base_enqueue(ctx, s, s.im[0].img, h, w, w, tmp, base)) ||
            (rc = sift_base_enqueue(ctx, s, s.im[1].img, h, w, w, tmp, base1)) ||
            (rc = sift_descriptors_listed_pair_enqueue(ctx, s, base, base1, h, w, s.im[0].edges, s.im[1].edges, usedL, usedR, used_cnt, nL,
                                                       nR, dL, dR)) ||
            (rc = match_expand_rows_enqueue(ctx, s, rp0, nL, n0, (int32_t *)s.pair_left.p)) ||
            (rc = sift_distances_enqueue(ctx, s, dL, dR, (const int32_t *)s.pair_left.p, (const int32_t *)s.col_idx.p, n0,
                                         p->sift_thr, dist, ok)) ||
            (rc = sift_and_flags_enqueue(ctx, s, ok, (const uint8_t *)s.keep.p, n0, both)))
            return rc;
        if ((rc = glue_rows_from_flags_enqueue(ctx, s, rp0, nL, ok, cnt, order)) || (rc = scan_counts(rpA, T_SIFT)) ||
            (rc = gt_eval(EBVO_GT_SIFT, rp0, nullptr, ok)))
            return rc;
        keep1 = both;
        conf0 = dist;
        s.sift_left_valid = true; // dL: the descriptors of every left TOED edge that has a candidate (ebvo_temporal_* reuse the final mates')
    }
    // 1. the kept NCC matches as a CSR list of right TOED edges with their scores (apply_NCC_Filtering's output, :597-607)
    if ((rc = glue_rows_from_flags_enqueue(ctx, s, rp0, nL, keep1, cnt, order)) || (rc = scan_counts(rpA, T_NCC)) ||
        (rc = glue_gather_rows_enqueue(ctx, s, rp0, cnt, order, rpA, nL, s.im[1].edges, (const int32_t *)s.col_idx.p, candA,
                                       (const double *)s.best.p, scoreA)) ||
        (conf0 && (rc = glue_gather_rows_enqueue(ctx, s, rp0, cnt, order, rpA, nL, nullptr, nullptr, nullptr, conf0, confA))) ||
        (rc = gt_eval(EBVO_GT_NCC, rp0, nullptr, keep1)))
        return rc;
    // 2. Best-Nearly-Best test on the NCC scores (:1440) ...
    if ((rc = glue_bnb_enqueue(ctx, s, rpA, nL, scoreA, p->bnb_ratio, 1, cnt, order)) || (rc = scan_counts(rpB, T_BNB)) ||
        (rc = glue_gather_rows_enqueue(ctx, s, rpA, cnt, order, rpB, nL, candA, nullptr, candB, scoreA, scoreB)) ||
        (conf0 && (rc = glue_gather_rows_enqueue(ctx, s, rpA, cnt, order, rpB, nL, nullptr, nullptr, nullptr, confA, confB))) ||
        (rc = gt_eval(EBVO_GT_BNB_NCC, rpB, candB, nullptr)))
        return rc;
    if (conf0)
    {
        // ... and on the SIFT distances, lower is better (:1452).  The survivors land in candA / rpA; the two sets of buffers
        // swap their roles instead of being copied back.
        if ((rc = glue_bnb_enqueue(ctx, s, rpB, nL, confB, p->bnb_sift, 0, cnt, order)) || (rc = scan_counts(rpA, T_BNB)) ||
            (rc = glue_gather_rows_enqueue(ctx, s, rpB, cnt, order, rpA, nL, candB, nullptr, candA, scoreB, scoreA)))
            return rc;
        std::swap(rpA, rpB);
        std::swap(candA, candB);
        std::swap(scoreA, scoreB);
        if ((rc = gt_eval(EBVO_GT_BNB_SIFT, rpB, candB, nullptr)))
            return rc;
    }
    const int32_t *d_nB = rpB + nL; // pairs that enter the refinement: a subset of the run's kept NCC matches
    const int64_t n_ref = s.result.n_matches < n0 ? (s.result.n_matches > 0 ? s.result.n_matches : 1) : n0;
    {
        // 3. epipolar shift (:1436) and 4. photometric refinement along the epipolar line (:1438)
        double *out = (double *)s.gn_out.p;
        if ((rc = match_expand_rows_enqueue(ctx, s, rpB, nL, n0, left_of)) ||
            (rc = glue_shift_enqueue(ctx, s, candB, (const double *)s.lines.p, left_of, n0, candC, d_nB)) ||
            (rc = glue_xy_enqueue(ctx, s, candC, (double *)s.gn_xy.p, n0, false, d_nB)) ||
            (rc = refine_gn_stereo_enqueue(ctx, s, s.im[0].img, s.im[1].img, nullptr, h, w, s.im[0].edges, nL,
                                           (const double *)s.lines.p, left_of, (const double *)s.gn_xy.p, nullptr, nullptr,
                                           nullptr, n_ref, p->gn.max_iter, p->gn.tol, p->gn.huber_delta, out, out + nz,
                                           out + 2 * nz, (uint8_t *)s.gn_valid.p, (int32_t *)s.gn_iters.p, out + 3 * nz, d_nB)) ||
            (rc = glue_xy_enqueue(ctx, s, candC, out + 3 * nz, n0, true, d_nB)) ||
            (rc = gt_eval(EBVO_GT_REFINE, rpB, candC, nullptr)))
            return rc;
        // 5. consolidate_redundant_edge_hypothesis(pairs, false, true) (:1483).  Against the signature (pairs, frame_idx,
        // b_do_epipolar_shift = true, b_do_clustering = true) this binds frame_idx = 0, shift = true, cluster = true: the
        // refined centres are shifted to the epipolar line AGAIN (:981-998) and clustered with b_cluster_by_orientation =
        // b_do_epipolar_shift = true (:1031); rows with one candidate are not skipped on the shift branch (:1001 is the
        // else branch only).  -> candA in the rows of rpA
        if ((rc = glue_shift_enqueue(ctx, s, candC, (const double *)s.lines.p, left_of, n0, candA, d_nB)) ||
            (rc = glue_cluster_enqueue(ctx, s, candA, rpB, nL, 1, 0, cnt, candB, cluster_of)) ||
            (rc = scan_counts(rpA, T_CLUSTERS)) ||
            (rc = glue_gather_rows_enqueue(ctx, s, rpB, cnt, nullptr, rpA, nL, candB, nullptr, candA, nullptr, nullptr)) ||
            (rc = gt_eval(EBVO_GT_CLUSTER, rpA, candA, nullptr)))
            return rc;
    }
    {
        // 6. second NCC pass on the cluster centres (:1500) -> keep2 / best2, 7. the best survivor of every row (:1513).
        // The normalised left patches (left_edge_patches, :578) are sampled here: the first pass keeps them in LDS only.
        if ((rc = match_patches_enqueue(ctx, s, ncc_img(s, 0), h, w, w, s.im[0].edges, nL, nullptr, 0, nullptr,
                                        (float *)s.patches_norm.p, (uint8_t *)s.patches_flag.p)) ||
            (rc = match_ncc_pairs_enqueue(ctx, s, ncc_img(s, 1), h, w, w, candA, rpA, nL, n0, (const float *)s.patches_norm.p,
                                          (const uint8_t *)s.patches_flag.p, p->ncc_thr, nullptr, best2, keep2, ncc_left,
                                          sincos2, rpA + nL)) ||
            (rc = glue_rows_from_flags_enqueue(ctx, s, rpA, nL, keep2, cnt, order)) || (rc = scan_counts(rpB, T_NCC2)) ||
            (rc = glue_gather_rows_enqueue(ctx, s, rpA, cnt, order, rpB, nL, candA, nullptr, candC, best2, scoreB)) ||
            (rc = gt_eval(EBVO_GT_NCC2, rpB, candC, nullptr)))
            return rc;
        if ((rc = glue_keep_best_enqueue(ctx, s, rpB, nL, scoreB, cnt, order)) || (rc = scan_counts(rpA, T_FINAL)) ||
            (rc = glue_final_pairs_enqueue(ctx, s, rpB, cnt, order, rpA, nL, s.im[0].edges, candC, scoreB, final_left,
                                           fin_l, fin_r, fin_score)) ||
            (rc = gt_eval(EBVO_GT_BEST, rpA, fin_r, nullptr)))
            return rc;
    }
    // 8. the rows of the output file (at most one final pair per left edge)
    if (calib && (rc = refine_finalize_pairs_enqueue(ctx, s, calib->K_left, calib->K_right, calib->R21, calib->T21, fin_l, fin_r,
                                                     nL, (double *)s.fin_out.p, tot + T_FINAL)))
        return rc;
    EBVO_HIP(ctx, hipMemcpyAsync(s.h_fin_tot, tot, sizeof(int32_t) * 8, hipMemcpyDeviceToHost, st));
    EBVO_HIP(ctx, hipEventRecord(s.ev_fin, st));
    return EBVO_OK;
}

extern "C" int ebvo_stereo_finalize_submit(ebvo_ctx *ctx, int slot, const ebvo_finalize_params *p, const ebvo_stereo_calib *calib)
{
    Slot *sp;
    if (!p || !(p->bnb_ratio >= 0) || !(p->ncc_thr == p->ncc_thr) || p->gn.max_iter < 1 || !(p->gn.tol >= 0) ||
        !(p->gn.huber_delta > 0) || (p->use_sift && (!(p->sift_thr > 0) || !(p->bnb_sift >= 0))) || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_run || s.in_flight || s.fin_in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc_f = drain_fetch(ctx, s))
        return rc_f;
    const FinalizeGridScope grid_scope(ctx, s);
    s.have_final = s.have_refined = false; // the refinement buffers are reused
    s.tq_n = -1;
    s.tq_final.n = -1;
    s.tq_trail = Slot::TqTrail();
    s.sift_left_valid = false;
    s.n_final = 0;
    s.final_has_rows = calib != nullptr;
    s.gt_fin_enq = s.gt_armed;
    s.gt_fin_sift = p->use_sift != 0;
    s.gt_fin_done = false;
    memset(s.h_fin_tot, 0, sizeof(int32_t) * 8);
    if (s.result.n_left == 0 || s.result.n_pairs == 0)
    {
        // armed: every stage of the chain holds an empty list on every row; (n, tp) = 0 and the totals of that (rows = the
        // focused rows), so that the record of a stage says what Evaluate_Stereo_Edge_Correspondences would (:332-335)
        for (int k = EBVO_GT_SIFT; s.gt_armed && s.gt_nL > 0 && k <= EBVO_GT_BEST; ++k)
        {
            int32_t *rows = (int32_t *)s.gt_rows.p + (size_t)k * 2 * s.gt_nL;
            EBVO_HIP(ctx, hipMemsetAsync(rows, 0, sizeof(int32_t) * 2 * (size_t)s.gt_nL, s.stream));
            if (int rc_g = gt_totals_enqueue(ctx, s, rows, (const uint8_t *)s.gt_flags.p + s.gt_nL, s.gt_nL,
                                             (unsigned long long *)s.gt_tot.p + (size_t)k * 8))
                return rc_g;
        }
        EBVO_HIP(ctx, hipEventRecord(s.ev_fin, s.stream)); // nothing to do: the wait returns zero counts
        s.fin_in_flight = true;
        return EBVO_OK;
    }
    int rc = finalize_enqueue(ctx, s, p, calib);
    if (rc)
    {
        (void)hipStreamSynchronize(s.stream); // part of the chain may be enqueued
        return rc;
    }
    s.fin_in_flight = true;
    return EBVO_OK;
}

extern "C" int ebvo_stereo_finalize_wait(ebvo_ctx *ctx, int slot, ebvo_finalize_counts *counts)
{
    Slot *sp;
    if (!counts || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.fin_in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    s.fin_in_flight = false;
    EBVO_HIP(ctx, hipEventSynchronize(s.ev_fin));
    const int32_t *t = s.h_fin_tot;
    memset(counts, 0, sizeof *counts);
    counts->n_sift = t[0];
    counts->n_ncc = t[1];
    counts->n_bnb = t[2];
    counts->n_clusters = t[3];
    counts->n_ncc2 = t[4];
    counts->n_final = t[5];
    s.n_final = t[5];
    s.have_final = true;
    s.gt_fin_done = s.gt_fin_enq;
    return EBVO_OK;
}

extern "C" int ebvo_stereo_finalize(ebvo_ctx *ctx, int slot, const ebvo_finalize_params *p, const ebvo_stereo_calib *calib,
                                    ebvo_finalize_counts *counts)
{
    if (!counts)
        return EBVO_ERR_ARG;
    int rc = ebvo_stereo_finalize_submit(ctx, slot, p, calib);
    return rc ? rc : ebvo_stereo_finalize_wait(ctx, slot, counts);
}

extern "C" int ebvo_stereo_fetch_final(ebvo_ctx *ctx, int slot, int32_t *left_index, ebvo_edge *right_edge, double *ncc_score,
                                       double *out16)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_final || s.in_flight)
        return EBVO_ERR_STATE;
    if (out16 && !s.final_has_rows)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)s.n_final;
    if (!n)
        return EBVO_OK;
    const size_t nz = (size_t)s.result.n_pairs, nLz = (size_t)s.result.n_left + 1;
    const int32_t *final_left = (const int32_t *)s.fin_i32.p + 3 * nLz;
    const ebvo_edge *fin_r = (const ebvo_edge *)s.fin_edges.p + 3 * nz + nLz;
    const double *fin_score = (const double *)s.fin_f64.p + 3 * nz;
    hipStream_t st = s.stream;
    if (left_index)
        EBVO_HIP(ctx, hipMemcpyAsync(left_index, final_left, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (right_edge)
        EBVO_HIP(ctx, hipMemcpyAsync(right_edge, fin_r, sizeof(ebvo_edge) * n, hipMemcpyDeviceToHost, st));
    if (ncc_score)
        EBVO_HIP(ctx, hipMemcpyAsync(ncc_score, fin_score, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (out16)
        EBVO_HIP(ctx, hipMemcpyAsync(out16, s.fin_out.p, sizeof(double) * 16 * n, hipMemcpyDeviceToHost, st));
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    return EBVO_OK;
}

extern "C" int ebvo_stereo_fetch_slot(ebvo_ctx *ctx, int slot, ebvo_edge *left, ebvo_edge *right, int32_t *row_ptr,
                                      int32_t *col_idx, double *sims, double *best, uint8_t *keep, float *left_patches)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_run || s.in_flight)
        return EBVO_ERR_STATE;
    if (sims && !s.have_sims)
    {
        ctx->last_error = "the pair was submitted with EBVO_PAIR_NO_SIMS: the four scores were not stored";
        return EBVO_ERR_STATE;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nL = (size_t)s.result.n_left, nR = (size_t)s.result.n_right, np = (size_t)s.result.n_pairs;
    hipStream_t st = s.stream;
    if (left && nL)
        EBVO_HIP(ctx, hipMemcpyAsync(left, s.im[0].edges, sizeof(ebvo_edge) * nL, hipMemcpyDeviceToHost, st));
    if (right && nR)
        EBVO_HIP(ctx, hipMemcpyAsync(right, s.im[1].edges, sizeof(ebvo_edge) * nR, hipMemcpyDeviceToHost, st));
    if (row_ptr)
        EBVO_HIP(ctx, hipMemcpyAsync(row_ptr, s.row_ptr.p, sizeof(int32_t) * (nL + 1), hipMemcpyDeviceToHost, st));
    if (col_idx && np)
        EBVO_HIP(ctx, hipMemcpyAsync(col_idx, s.col_idx.p, sizeof(int32_t) * np, hipMemcpyDeviceToHost, st));
    if (sims && np)
        EBVO_HIP(ctx, hipMemcpyAsync(sims, s.sims.p, sizeof(double) * 4 * np, hipMemcpyDeviceToHost, st));
    if (best && np)
        EBVO_HIP(ctx, hipMemcpyAsync(best, s.best.p, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    if (keep && np)
        EBVO_HIP(ctx, hipMemcpyAsync(keep, s.keep.p, np, hipMemcpyDeviceToHost, st));
    if (left_patches && nL)
    {
        // the pipeline keeps only the normalised banks; the raw left patches (what the reference stores per match,
        // src/Stereo_Matches.cpp:1622) are sampled when they are asked for
        int rc = match_patches_enqueue(ctx, s, ncc_img(s, 0), s.cur_h, s.cur_w, s.cur_w, s.im[0].edges, (int)nL, nullptr, 0,
                                       (float *)s.patches_raw.p, nullptr, nullptr);
        if (rc)
            return rc;
        EBVO_HIP(ctx, hipMemcpyAsync(left_patches, s.patches_raw.p, sizeof(float) * 98 * nL, hipMemcpyDeviceToHost, st));
    }
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    return EBVO_OK;
}




// ---- fixed-scale SIFT descriptors and the descriptor-distance score ---------------------------------------------------
extern "C" int ebvo_sift_descriptors(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, const ebvo_edge *edges,
                                     int n, float *desc)
{
    if (!ctx || !img || n < 0 || (n > 0 && (!edges || !desc)))
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (n == 0)
        return EBVO_OK;
    const size_t npx = (size_t)h * w, nz = (size_t)n;
    if (hc.image(0, img, h, w, stride) || hc.grow(s.sift_img, sizeof(float) * 2 * npx) || hc.grow(s.scratch_b, sizeof(ebvo_edge) * nz) ||
        hc.grow(s.sift_f32, sizeof(float) * 256 * nz) || hc.up(s.scratch_b.p, edges, sizeof(ebvo_edge) * nz))
        return hc.rc;
    float *tmp = (float *)s.sift_img.p, *base = tmp + npx;
    int rc;
    if ((rc = sift_base_enqueue(ctx, s, s.im[0].img, h, w, w, tmp, base)) ||
        (rc = sift_descriptors_enqueue(ctx, s, base, h, w, (const ebvo_edge *)s.scratch_b.p, n, (float *)s.sift_f32.p, nullptr)))
        return rc;
    hc.down(desc, s.sift_f32.p, sizeof(float) * 256 * nz);
    return hc.finish();
}

extern "C" int ebvo_sift_min_distances(ebvo_ctx *ctx, const float *left_desc, int nL, const float *cand_desc,
                                       const int32_t *row_ptr, double *dist)
{
    int64_t np = 0;
    if (!ctx || check_csr(row_ptr, nL, &np) || (np > 0 && (!left_desc || !cand_desc || !dist)))
        return EBVO_ERR_ARG;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (np == 0)
        return EBVO_OK;
    const size_t npz = (size_t)np, nLz = (size_t)nL;
    if (hc.grow(s.sift_f32, sizeof(float) * 256 * (npz + nLz)) || hc.grow(s.sift_desc, 256 * (npz + nLz)) ||
        hc.grow(s.row_ptr, sizeof(int32_t) * (nLz + 1)) || hc.grow(s.pair_left, sizeof(int32_t) * npz) ||
        hc.grow(s.sift_dist, sizeof(double) * npz))
        return hc.rc;
    float *fl = (float *)s.sift_f32.p, *fc = fl + 256 * nLz;
    uint8_t *ul = (uint8_t *)s.sift_desc.p, *uc = ul + 256 * nLz;
    if (hc.up(fl, left_desc, sizeof(float) * 256 * nLz) || hc.up(fc, cand_desc, sizeof(float) * 256 * npz) ||
        hc.up(s.row_ptr.p, row_ptr, sizeof(int32_t) * (nLz + 1)))
        return hc.rc;
    int rc;
    if ((rc = sift_to_u8_enqueue(ctx, s, fl, (int64_t)(256 * (nLz + npz)), ul)) ||
        (rc = match_expand_rows_enqueue(ctx, s, (const int32_t *)s.row_ptr.p, nL, np, (int32_t *)s.pair_left.p)) ||
        (rc = sift_distances_enqueue(ctx, s, ul, uc, (const int32_t *)s.pair_left.p, nullptr, np, EBVO_SIFT_THRESHOLD,
                                     (double *)s.sift_dist.p, nullptr)))
        return rc;
    hc.down(dist, s.sift_dist.p, sizeof(double) * npz);
    return hc.finish();
}

// ---- input side: cv::undistort ---------------------------------------------------------------------------------
extern "C" int ebvo_undistort(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, const double K[4],
                              const double *dist, int n_dist, uint8_t *out, ptrdiff_t out_stride)
{
    if (!ctx || !img || !out || !K || n_dist < 0 || n_dist > 5 || (n_dist > 0 && !dist) || out_stride < w)
        return EBVO_ERR_ARG;
    if (int rc = check_size(ctx, h, w))
        return rc;
    HostCall hc(ctx, HostCall::PAIR_BUFFERS);
    if (hc.rc)
        return hc.rc;
    Slot &s = hc.slot();
    if (hc.image(0, img, h, w, stride))
        return hc.rc;
    if (int rc = refine_undistort_enqueue(ctx, s, s.im[0].img, w, h, w, K, dist, n_dist, s.im[0].undist_xs, s.im[1].img, w))
        return rc;
    hc.down_rows(out, (size_t)out_stride, s.im[1].img, (size_t)w, (size_t)h);
    return hc.finish();
}

extern "C" int ebvo_stereo_set_undistort(ebvo_ctx *ctx, const ebvo_undistort_params *p)
{
    if (ctx)
        ++ctx->graph_gen; // the coefficients are launch arguments of a captured chain

    if (!ctx || (p && (p->n_dist < 0 || p->n_dist > 5)))
        return EBVO_ERR_ARG;
    for (Slot *s : ctx->slots)
        if (s->in_flight)
            return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (!p)
    {
        ctx->undist_on = false;
        return EBVO_OK;
    }
    for (Slot *s : ctx->slots)
        for (int k = 0; k < 2; ++k)
            if (!s->im[k].raw_base)
            {
                const size_t bytes = (size_t)ctx->max_h * ctx->max_w + 128;
                if (hipMalloc(&s->im[k].raw_base, bytes) != hipSuccess)
                {
                    (void)hipGetLastError();
                    return EBVO_ERR_NOMEM;
                }
                EBVO_HIP(ctx, hipMemsetAsync(s->im[k].raw_base, 0, bytes, s->stream));
                EBVO_HIP(ctx, hipStreamSynchronize(s->stream));
                s->im[k].raw = s->im[k].raw_base + 64;
            }
    ctx->undist = *p;
    ctx->undist_on = true;
    for (Slot *s : ctx->slots) // pairs uploaded before the switch went to img: they must be uploaded again
        s->have_pair = s->have_run = s->have_refined = s->have_final = s->gt_armed = false;
    return EBVO_OK;
}


// ---- temporal quads against the keyframe ---------------------------------------------------------------------------
extern "C" void ebvo_temporal_default_params(ebvo_temporal_params *p)
{
    if (!p)
        return;
    memset(p, 0, sizeof *p);
    p->cell_size = 15;
    p->grid_radius = 30.0;
    p->orient_thr_deg = 10.0;
    p->ncc_thr = EBVO_NCC_THRESH_TEMPORAL;
    p->stages = 0;
    p->sift_thr = 200.0; // src/Temporal_Matches.cpp:196
    p->bnb_ncc = 0.8;    // :200
    p->bnb_sift = 0.8;   // :204
    ebvo_gn_default_params(&p->gn); // 20, 1e-3, 3.0 (:612, :615)
}

// the final mates of a finalized slot: left edges, right centre edges (carved by ebvo_stereo_finalize)
static void final_mates(Slot &s, const ebvo_edge **fl, const ebvo_edge **fr)
{
    const size_t nz = (size_t)s.result.n_pairs, nLz = (size_t)s.result.n_left + 1;
    *fl = (const ebvo_edge *)s.fin_edges.p + 3 * nz;
    *fr = *fl + nLz;
}

// SIFT descriptors of n stereo mates of the slot's pair: left edges on the undistorted left image, right edges on the
// undistorted right image (the octave base of each image is rebuilt here: one separable blur per image)
static int mate_descriptors(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_L, const ebvo_edge *d_R, int n, uint8_t *d_descL,
                            uint8_t *d_descR)
{
    const int h = s.cur_h, w = s.cur_w;
    const size_t npx = (size_t)h * w;
    int rc;
    if ((rc = ebvo_grow(ctx, s, s.sift_img, sizeof(float) * 2 * npx)))
        return rc;
    float *tmp = (float *)s.sift_img.p, *base = tmp + npx;
    // a mate's left edge IS its left TOED edge: if ebvo_stereo_finalize ran the SIFT stages on this pair, the descriptors of
    // every left TOED edge are still there and the mates' are picked from them
    const size_t nLz = (size_t)s.result.n_left + 1;
    if (s.sift_left_valid && s.have_final && d_L == (const ebvo_edge *)s.fin_edges.p + 3 * (size_t)s.result.n_pairs)
    {
        if ((rc = sift_gather_enqueue(ctx, s, (const uint8_t *)s.sift_desc.p, (const int32_t *)s.fin_i32.p + 3 * nLz, n, d_descL)))
            return rc;
    }
    else if ((rc = sift_base_enqueue(ctx, s, s.im[0].img, h, w, w, tmp, base)) ||
             (rc = sift_descriptors_enqueue(ctx, s, base, h, w, d_L, n, nullptr, d_descL)))
        return rc;
    if ((rc = sift_base_enqueue(ctx, s, s.im[1].img, h, w, w, tmp, base)) ||
        (rc = sift_descriptors_enqueue(ctx, s, base, h, w, d_R, n, nullptr, d_descR)))
        return rc;
    return EBVO_OK;
}

// what a slot needs to become the keyframe (ebvo_temporal_set_keyframe, ebvo_temporal_promote_keyframe)
static int keyframe_slot_state(ebvo_ctx *ctx, const Slot &s)
{
    if (!s.have_final || s.in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    // a match in flight in ANY slot reads the stored keyframe (ctx->kf_*) on its own stream, and its wait runs the chain
    // against it: the store is neither overwritten nor re-allocated under it
    for (const Slot *o : ctx->slots)
        if (o->tq_in_flight)
        {
            ctx->last_error = "a temporal match is in flight in another slot (ebvo_temporal_match_wait first): the keyframe stays";
            return EBVO_ERR_STATE;
        }
    return EBVO_OK;
}

// the slot's final mates, patches, descriptors and images into the keyframe store; the depth state back to the prior.  Waits.
static int keyframe_install(ebvo_ctx *ctx, Slot &s)
{
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc_f = drain_fetch(ctx, s))
        return rc_f;
    for (Slot *o : ctx->slots) // a pending pose prior (ebvo_temporal_set_prior) was given for the keyframe that goes
        o->tq_prior_next.on = false;
    const size_t n = (size_t)s.n_final;
    if (n > ctx->kf_cap)
    {
        EBVO_HIP(ctx, hipDeviceSynchronize());
        for (void *p : {(void *)ctx->kf_L, (void *)ctx->kf_R, (void *)ctx->kf_Ln, (void *)ctx->kf_Rn, (void *)ctx->kf_Lf, (void *)ctx->kf_Rf,
                        (void *)ctx->kf_Ld, (void *)ctx->kf_Rd})
            (void)hipFree(p);
        ctx->kf_L = ctx->kf_R = nullptr;
        ctx->kf_Ln = ctx->kf_Rn = nullptr;
        ctx->kf_Lf = ctx->kf_Rf = nullptr;
        ctx->kf_Ld = ctx->kf_Rd = nullptr;
        ctx->kf_cap = 0;
        const size_t cap = n + n / 4 + 64;
        if (hipMalloc(&ctx->kf_L, sizeof(ebvo_edge) * cap) != hipSuccess || hipMalloc(&ctx->kf_R, sizeof(ebvo_edge) * cap) != hipSuccess ||
            hipMalloc(&ctx->kf_Ln, sizeof(float) * 98 * cap) != hipSuccess || hipMalloc(&ctx->kf_Rn, sizeof(float) * 98 * cap) != hipSuccess ||
            hipMalloc(&ctx->kf_Lf, 2 * cap) != hipSuccess || hipMalloc(&ctx->kf_Rf, 2 * cap) != hipSuccess ||
            hipMalloc(&ctx->kf_Ld, 256 * cap) != hipSuccess || hipMalloc(&ctx->kf_Rd, 256 * cap) != hipSuccess)
        {
            (void)hipGetLastError();
            ctx->last_error = "hipMalloc failed (keyframe store)";
            return EBVO_ERR_NOMEM;
        }
        ctx->kf_cap = cap;
    }
    ctx->kf_n = (int)n;
    ctx->kf_depth_fresh = true; // the new keyframe's mates are at the prior
    ctx->kf_promoted = false;
    ++ctx->kf_gen; // quads matched against the previous keyframe no longer belong to ctx->kf_L / kf_R
    {
        // the keyframe's undistorted images stay with it: the photometric refinement of the quads samples them
        const size_t bytes = (size_t)s.cur_h * s.cur_w;
        if (bytes > ctx->kf_img_bytes)
        {
            EBVO_HIP(ctx, hipDeviceSynchronize());
            (void)hipFree(ctx->kf_imgL);
            (void)hipFree(ctx->kf_imgR);
            ctx->kf_imgL = ctx->kf_imgR = nullptr;
            ctx->kf_img_bytes = 0;
            if (hipMalloc(&ctx->kf_imgL, bytes) != hipSuccess || hipMalloc(&ctx->kf_imgR, bytes) != hipSuccess)
            {
                (void)hipGetLastError();
                ctx->last_error = "hipMalloc failed (keyframe images)";
                return EBVO_ERR_NOMEM;
            }
            ctx->kf_img_bytes = bytes;
        }
        EBVO_HIP(ctx, hipMemcpyAsync(ctx->kf_imgL, s.im[0].img, bytes, hipMemcpyDeviceToDevice, s.stream));
        EBVO_HIP(ctx, hipMemcpyAsync(ctx->kf_imgR, s.im[1].img, bytes, hipMemcpyDeviceToDevice, s.stream));
        ctx->kf_h = s.cur_h;
        ctx->kf_w = s.cur_w;
    }
    if (n == 0)
    {
        EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
        return EBVO_OK;
    }
    const ebvo_edge *fl, *fr;
    final_mates(s, &fl, &fr);
    int rc;
    EBVO_HIP(ctx, hipMemcpyAsync(ctx->kf_L, fl, sizeof(ebvo_edge) * n, hipMemcpyDeviceToDevice, s.stream));
    EBVO_HIP(ctx, hipMemcpyAsync(ctx->kf_R, fr, sizeof(ebvo_edge) * n, hipMemcpyDeviceToDevice, s.stream));
    // left_edge_patches: raw left image (src/Stereo_Matches.cpp:578, :1621); right_edge_patches: undistorted right (:1622)
    if ((rc = match_patches_enqueue(ctx, s, ncc_img(s, 0), s.cur_h, s.cur_w, s.cur_w, ctx->kf_L, (int)n, nullptr, 0, nullptr, ctx->kf_Ln,
                                    ctx->kf_Lf)) ||
        (rc = match_patches_enqueue(ctx, s, s.im[1].img, s.cur_h, s.cur_w, s.cur_w, ctx->kf_R, (int)n, nullptr, 0, nullptr, ctx->kf_Rn,
                                    ctx->kf_Rf)))
        return rc;
    // left_edge_descriptors (augment_Edge_Data, src/Stereo_Matches.cpp:655-689: the left TOED edge on the undistorted left
    // image) and right_edge_descriptors (finalize_stereo_edge_mates, :1627-1635: the final right edge on the undistorted
    // right image) of every mate
    if ((rc = mate_descriptors(ctx, s, fl, fr, (int)n, ctx->kf_Ld, ctx->kf_Rd)))
        return rc;
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    return EBVO_OK;
}

extern "C" int ebvo_temporal_set_keyframe(ebvo_ctx *ctx, int slot)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    if (int rc = keyframe_slot_state(ctx, *sp))
        return rc;
    if (int rc = keyframe_install(ctx, *sp))
        return rc;
    // the sequence frame is this keyframe's
    for (int i = 0; i < 9; ++i)
        ctx->kf_Rk[i] = i % 4 == 0 ? 1.0 : 0.0;
    ctx->kf_tk[0] = ctx->kf_tk[1] = ctx->kf_tk[2] = 0.0;
    return EBVO_OK;
}

// developer key 22 holds for the launches of temporal_stage0_enqueue and temporal_chain only: the helpers they share with
// the stereo chain (patches, glue, SIFT, refinement) read Slot::tq_blocks, which is zero outside this scope
struct TemporalGridScope
{
    Slot &s;
    TemporalGridScope(const ebvo_ctx *ctx, Slot &slot) : s(slot) { s.tq_blocks = ctx->temporal_blocks; }
    ~TemporalGridScope() { s.tq_blocks = 0; }
};

// get_Temporal_Edge_Pairs_from_Quads after the NCC filter (src/Temporal_Matches.cpp:196-215) on the candidate quads of the
// slot's pair: rp / col / quad_kf / sim_l / keep are the CSR candidate lists, the current-frame mate and the keyframe mate
// of every candidate, its left NCC maximum and the NCC keep flag, as ebvo_temporal_match left them on the device.
static int temporal_chain(ebvo_ctx *ctx, Slot &s, const ebvo_temporal_params &P, const int32_t *rp, const int32_t *col,
                          const int32_t *quad_kf, const double *sim_l, const uint8_t *keep, int n_kf, const ebvo_edge *cfL,
                          const ebvo_edge *cfR, int n_cf, int64_t n_kept, ebvo_temporal_counts *counts)
{
    const int h = s.cur_h, w = s.cur_w;
    const size_t nk1 = (size_t)n_kf + 1, nK = (size_t)(n_kept > 0 ? n_kept : 1), ncz = (size_t)n_cf;
    hipStream_t st = s.stream;
    int rc;
    const TemporalGridScope grid_scope(ctx, s);
    // one buffer, carved: two quad sets (ping-pong), row bookkeeping, refinement and clustering arrays, the final lists
    struct QuadSet
    {
        int32_t *rp, *cf, *kf;
        double *simL, *siftL, *siftR;
    } A, B;
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 63) & ~(size_t)63;
        return o;
    };
    size_t o_set[2][6];
    for (int k = 0; k < 2; ++k)
    {
        o_set[k][0] = carve(sizeof(int32_t) * nk1);
        o_set[k][1] = carve(sizeof(int32_t) * nK);
        o_set[k][2] = carve(sizeof(int32_t) * nK);
        o_set[k][3] = carve(sizeof(double) * nK);
        o_set[k][4] = carve(sizeof(double) * nK);
        o_set[k][5] = carve(sizeof(double) * nK);
    }
    // `order` is indexed like the INPUT list of a selection: the first one selects from all nq candidate quads
    const size_t nq = (size_t)(s.tq_n > 0 ? s.tq_n : 1);
    const size_t o_cnt = carve(sizeof(int32_t) * (nk1 + 1)), o_order = carve(sizeof(int32_t) * (nq > nK ? nq : nK)),
                 o_idx = carve(sizeof(int32_t) * nK),
                 o_ok = carve(3 * nK), o_desc = carve(512 * ncz), o_kfe = carve(sizeof(ebvo_edge) * 2 * nK),
                 o_cfe = carve(sizeof(ebvo_edge) * 2 * nK), o_init = carve(sizeof(double) * 4 * nK),
                 o_disp = carve(sizeof(double) * 4 * nK), o_score = carve(sizeof(double) * 2 * nK), o_valid = carve(3 * nK),
                 o_iters = carve(sizeof(int32_t) * 2 * nK), o_cen = carve(sizeof(ebvo_edge) * 2 * nK),
                 o_centres = carve(sizeof(ebvo_edge) * nK), o_clof = carve(sizeof(int32_t) * nK),
                 o_frp = carve(sizeof(int32_t) * nk1), o_fsrc = carve(sizeof(int32_t) * nK), o_fcf = carve(sizeof(int32_t) * nK),
                 o_fL = carve(sizeof(ebvo_edge) * nK), o_fR = carve(sizeof(ebvo_edge) * nK), o_fd = carve(sizeof(double) * 4 * nK),
                 o_fvalid = carve(nK);
    // the stage trail (ebvo_temporal_keep_stages), behind everything else: room for the SIFT-stage list, which the BNB-SIFT
    // compaction overwrites
    Slot::TqTrail &T = s.tq_trail;
    const size_t o_trp = T.on ? carve(sizeof(int32_t) * nk1) : 0, o_tcf = T.on ? carve(sizeof(int32_t) * nK) : 0;
    if ((rc = ebvo_grow(ctx, s, s.tq_chain, off + 64)))
        return rc;
    char *base = (char *)s.tq_chain.p;
    QuadSet *sets[2] = {&A, &B};
    for (int k = 0; k < 2; ++k)
    {
        sets[k]->rp = (int32_t *)(base + o_set[k][0]);
        sets[k]->cf = (int32_t *)(base + o_set[k][1]);
        sets[k]->kf = (int32_t *)(base + o_set[k][2]);
        sets[k]->simL = (double *)(base + o_set[k][3]);
        sets[k]->siftL = (double *)(base + o_set[k][4]);
        sets[k]->siftR = (double *)(base + o_set[k][5]);
    }
    int32_t *cnt = (int32_t *)(base + o_cnt), *order = (int32_t *)(base + o_order), *idx = (int32_t *)(base + o_idx);
    uint8_t *okL = (uint8_t *)(base + o_ok), *okR = okL + nK, *ok = okR + nK;
    uint8_t *cf_Ld = (uint8_t *)(base + o_desc), *cf_Rd = cf_Ld + 256 * ncz;
    auto scan_counts = [&](int32_t *rp_out, int32_t *total, int64_t known = -1) -> int {
        int r = ebvo_device_scan(ctx, s, cnt, rp_out, n_kf, nullptr, 1, n_kf + 1);
        if (r || known >= 0) // (a total the host already holds is not read back: one synchronisation less)
        {
            *total = (int32_t)(known >= 0 ? known : 0);
            return r;
        }
        return read_i32(ctx, s, rp_out + n_kf, total);
    };
    // select rows of `from` (counts / order just formed against from.rp) into `to`
    auto compact = [&](const QuadSet &from, QuadSet &to, int32_t *total, bool with_sift, int64_t known = -1) -> int {
        int r;
        if ((r = scan_counts(to.rp, total, known)) || *total == 0)
            return r;
        if ((r = glue_row_index_enqueue(ctx, s, from.rp, cnt, order, to.rp, n_kf, idx)))
            return r;
        GlueGather g;
        g.i_src[0] = from.cf, g.i_dst[0] = to.cf;
        g.i_src[1] = from.kf, g.i_dst[1] = to.kf;
        g.d_src[0] = from.simL, g.d_dst[0] = to.simL;
        if (with_sift)
        {
            g.d_src[1] = from.siftL, g.d_dst[1] = to.siftL;
            g.d_src[2] = from.siftR, g.d_dst[2] = to.siftR;
        }
        return glue_gather_enqueue(ctx, s, idx, *total, g);
    };
    auto trail_set = [&](int stage, const int32_t *t_rp, const int32_t *t_cf, int64_t n) {
        T.rp[stage - EBVO_TGT_SIFT] = t_rp;
        T.cf[stage - EBVO_TGT_SIFT] = t_cf;
        T.n[stage - EBVO_TGT_SIFT] = n;
    };
    // nothing left: an empty final list; the stages from `first_unreached` on ran on empty rows (the trail lists them empty)
    auto finish_empty = [&](int first_unreached) -> int {
        s.tq_final.rp = (int32_t *)(base + o_frp);
        EBVO_HIP(ctx, hipMemsetAsync(s.tq_final.rp, 0, sizeof(int32_t) * nk1, st));
        EBVO_HIP(ctx, hipStreamSynchronize(st));
        s.tq_final.n = 0;
        if (T.on)
        {
            for (int k = first_unreached; k <= EBVO_TGT_REFINE; ++k)
                trail_set(k, s.tq_final.rp, nullptr, 0);
            T.lists = true;
        }
        return EBVO_OK;
    };
    // 0. the quads that passed the NCC filter
    int32_t n0 = 0;
    {
        QuadSet G0{const_cast<int32_t *>(rp), const_cast<int32_t *>(col), const_cast<int32_t *>(quad_kf), const_cast<double *>(sim_l),
                   nullptr, nullptr};
        // (their number came with the NCC counts: n_kept)
        if ((rc = glue_rows_from_flags_enqueue(ctx, s, rp, n_kf, keep, cnt, order)) || (rc = compact(G0, A, &n0, false, n_kept)))
            return rc;
    }
    if (n0 == 0)
        return finish_empty(EBVO_TGT_SIFT);
    // 1. apply_SIFT_filtering_quads (:471-515): the smaller of the four descriptor distances of the left edges AND of the right
    // edges below the threshold; the distances become the quad's SIFT scores
    if ((rc = mate_descriptors(ctx, s, cfL, cfR, n_cf, cf_Ld, cf_Rd)) ||
        (rc = sift_distances_enqueue(ctx, s, ctx->kf_Ld, cf_Ld, A.kf, A.cf, n0, P.sift_thr, A.siftL, okL)) ||
        (rc = sift_distances_enqueue(ctx, s, ctx->kf_Rd, cf_Rd, A.kf, A.cf, n0, P.sift_thr, A.siftR, okR)) ||
        (rc = sift_and_flags_enqueue(ctx, s, okL, okR, n0, ok)) || (rc = glue_rows_from_flags_enqueue(ctx, s, A.rp, n_kf, ok, cnt, order)))
        return rc;
    int32_t n1 = 0;
    if ((rc = compact(A, B, &n1, true)))
        return rc;
    counts->n_sift = n1;
    if (n1 == 0)
        return finish_empty(EBVO_TGT_SIFT);
    if (T.on)
    {
        int32_t *t_rp = (int32_t *)(base + o_trp), *t_cf = (int32_t *)(base + o_tcf);
        EBVO_HIP(ctx, hipMemcpyAsync(t_rp, B.rp, sizeof(int32_t) * nk1, hipMemcpyDeviceToDevice, st));
        EBVO_HIP(ctx, hipMemcpyAsync(t_cf, B.cf, sizeof(int32_t) * (size_t)n1, hipMemcpyDeviceToDevice, st));
        trail_set(EBVO_TGT_SIFT, t_rp, t_cf, n1);
    }
    // 2. apply_best_nearly_best_filtering_quads on the left NCC scores, then on the left SIFT scores (:517-570): rows of two or
    // more quads come out sorted by the score
    int32_t n2 = 0, n3 = 0;
    if ((rc = glue_bnb_enqueue(ctx, s, B.rp, n_kf, B.simL, P.bnb_ncc, 1 | 2, cnt, order)) || (rc = compact(B, A, &n2, true)))
        return rc;
    counts->n_bnb_ncc = n2;
    if ((rc = glue_bnb_enqueue(ctx, s, A.rp, n_kf, A.siftL, P.bnb_sift, 0 | 2, cnt, order)) || (rc = compact(A, B, &n3, true)))
        return rc;
    counts->n_bnb_sift = n3;
    if (T.on) // both lists stay where they are: nothing below writes set A, B's offsets or B's mates
    {
        trail_set(EBVO_TGT_BNB_NCC, A.rp, A.cf, n2);
        trail_set(EBVO_TGT_BNB_SIFT, B.rp, B.cf, n3);
    }
    if (n3 == 0)
        return finish_empty(EBVO_TGT_BNB_SIFT);
    // 3. apply_photometric_refinement_quads (:572-634): both cameras of every quad, keyframe image against the current image
    // (undistorted), gradients of the current image; the quad's centres move where the refinement is valid
    const size_t n3z = (size_t)n3;
    ebvo_edge *kfeL = (ebvo_edge *)(base + o_kfe), *kfeR = kfeL + n3z, *cfeL = (ebvo_edge *)(base + o_cfe), *cfeR = cfeL + n3z;
    double *initL = (double *)(base + o_init), *initR = initL + 2 * n3z, *dispL = (double *)(base + o_disp), *dispR = dispL + 2 * n3z;
    double *scoreL = (double *)(base + o_score), *scoreR = scoreL + n3z;
    uint8_t *validL = (uint8_t *)(base + o_valid), *validR = validL + n3z, *valid = validR + n3z;
    int32_t *itersL = (int32_t *)(base + o_iters); // the second camera's counts follow at + n3z (one batch, refine_gn_temporal_enqueue)
    ebvo_edge *cenL = (ebvo_edge *)(base + o_cen), *cenR = cenL + n3z;
    if ((rc = glue_quad_refine_inputs_enqueue(ctx, s, ctx->kf_L, B.kf, cfL, B.cf, n3, kfeL, cfeL, initL)) ||
        (rc = glue_quad_refine_inputs_enqueue(ctx, s, ctx->kf_R, B.kf, cfR, B.cf, n3, kfeR, cfeR, initR)) ||
        // both cameras in one batch: items 0 .. n3 - 1 the left images, n3 .. 2 n3 - 1 the right ones (the arrays are contiguous)
        (rc = refine_gn_temporal_enqueue(ctx, s, ctx->kf_imgL, s.im[0].img, nullptr, h, w, kfeL, cfeL, initL, 2 * (int64_t)n3,
                                         P.gn.max_iter, P.gn.tol, P.gn.huber_delta, dispL, scoreL, validL, itersL, n3, ctx->kf_imgR,
                                         s.im[1].img, nullptr)) ||
        (rc = glue_quad_apply_refine_enqueue(ctx, s, kfeL, cfeL, dispL, validL, kfeR, cfeR, dispR, validR, n3, cenL, cenR, valid)))
        return rc;
    unsigned long long *d_nvalid = (unsigned long long *)(base + o_ok); // (the SIFT flags are no longer needed)
    EBVO_HIP(ctx, hipMemsetAsync(d_nvalid, 0, sizeof *d_nvalid, st));
    if ((rc = match_count_flags_enqueue(ctx, s, valid, n3, d_nvalid)))
        return rc;
    // 4. apply_temporal_edge_clustering_quads (:636-733): EdgeClusterer by orientation on the refined left edges of every row of
    // two or more quads, the right centre and the record of a merged quad from its members
    ebvo_edge *centres = (ebvo_edge *)(base + o_centres);
    int32_t *cluster_of = (int32_t *)(base + o_clof);
    Slot::TqFinal F;
    F.rp = (int32_t *)(base + o_frp);
    int32_t *fsrc = (int32_t *)(base + o_fsrc);
    F.cf = (int32_t *)(base + o_fcf);
    F.L = (ebvo_edge *)(base + o_fL);
    F.R = (ebvo_edge *)(base + o_fR);
    F.ncc = (double *)(base + o_fd);
    int32_t n4 = 0;
    if ((rc = glue_cluster_enqueue(ctx, s, cenL, B.rp, n_kf, 1, 1, cnt, centres, cluster_of)) || (rc = scan_counts(F.rp, &n4)))
        return rc;
    const size_t n4z = (size_t)n4;
    F.sift = F.ncc + n4z;
    F.sL = F.sift + n4z;
    F.sR = F.sL + n4z;
    F.valid = (uint8_t *)(base + o_fvalid);
    if ((rc = glue_quad_cluster_post_enqueue(ctx, s, B.rp, n_kf, cnt, cluster_of, centres, cenL, cenR, F.rp, F.L, F.R, fsrc)))
        return rc;
    {
        GlueGather g;
        g.i_src[0] = B.cf, g.i_dst[0] = F.cf;
        g.d_src[0] = B.simL, g.d_dst[0] = F.ncc;
        g.d_src[1] = B.siftL, g.d_dst[1] = F.sift;
        g.d_src[2] = scoreL, g.d_dst[2] = F.sL;
        g.d_src[3] = scoreR, g.d_dst[3] = F.sR;
        g.b_src[0] = valid, g.b_dst[0] = F.valid;
        if ((rc = glue_gather_enqueue(ctx, s, fsrc, n4, g)))
            return rc;
    }
    unsigned long long nvalid = 0;
    EBVO_HIP(ctx, hipMemcpyAsync(s.h_result, d_nvalid, sizeof nvalid, hipMemcpyDeviceToHost, st));
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    memcpy(&nvalid, s.h_result, sizeof nvalid);
    counts->n_refined_valid = (int64_t)nvalid;
    counts->n_final = n4;
    s.tq_final.rp = F.rp;
    s.tq_final.cf = F.cf;
    s.tq_final.L = F.L;
    s.tq_final.R = F.R;
    s.tq_final.ncc = F.ncc;
    s.tq_final.sift = F.sift;
    s.tq_final.sL = F.sL;
    s.tq_final.sR = F.sR;
    s.tq_final.valid = F.valid;
    s.tq_final.n = n4;
    if (T.on)
    {
        trail_set(EBVO_TGT_REFINE, B.rp, B.cf, n3);
        T.cenL = cenL;
        T.cenR = cenR;
        T.lists = true;
    }
    return EBVO_OK;
}

// where the arrays of a match made under a prior lie in the slot's two buffers
static TemporalPrior temporal_prior_view(const Slot &s)
{
    const size_t nz = (size_t)s.tq_n_kf;
    TemporalPrior Q;
    Q.live = (const uint8_t *)s.tq_prior_live.p;
    Q.pl = (const double *)s.tq_prior_geom.p;
    Q.pr = Q.pl + 2 * nz;
    Q.ol = Q.pr + 2 * nz;
    Q.orr = Q.ol + nz;
    Q.use_orientation = s.tq_prior.P.use_orientation != 0;
    return Q;
}

// The projection of the slot's prior (s.tq_prior) for the s.tq_n_kf keyframe mates, enqueued on the slot's stream: live,
// both projections and both mapped orientations, against the CURRENT frame's size.
static int temporal_prior_enqueue(ebvo_ctx *ctx, Slot &s, TemporalPrior *out)
{
    const size_t nz = (size_t)s.tq_n_kf;
    int rc;
    if ((rc = ebvo_grow(ctx, s, s.tq_prior_geom, sizeof(double) * 6 * nz + 64)) || (rc = ebvo_grow(ctx, s, s.tq_prior_live, nz + 64)))
        return rc;
    const TemporalPrior Q = temporal_prior_view(s);
    const Slot::TqPrior &pr = s.tq_prior;
    if ((rc = tprior_project_enqueue(ctx, s, ctx->kf_L, ctx->kf_R, s.tq_n_kf, pr.R, pr.t, &pr.calib, pr.P.img_margin, s.cur_w, s.cur_h,
                                     const_cast<uint8_t *>(Q.live), const_cast<double *>(Q.pl), const_cast<double *>(Q.pr),
                                     const_cast<double *>(Q.ol), const_cast<double *>(Q.orr))))
        return rc;
    if (out)
        *out = Q;
    return EBVO_OK;
}

// Candidate quads + NCC of the slot's final mates against the keyframe's.  The buffers indexed by candidate quad are sized
// for a CAPACITY (s.tq_cap: what the last frame needed, with headroom), every kernel takes the number of quads from the
// device (the last entry of the scanned row offsets), and the two counts -- candidates, kept -- travel to page-locked memory
// behind the last kernel: no host synchronisation between the stages.  Only a first frame (no capacity yet) or a frame
// with more candidates than the capacity reads the count back first.
static int temporal_stage0_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_temporal_params *p, bool size_first)
{
    const int n_kf = ctx->kf_n, n_cf = s.n_final, h = s.cur_h, w = s.cur_w;
    int rc;
    const TemporalGridScope grid_scope(ctx, s);
    const size_t nk1 = (size_t)n_kf + 1;
    if ((rc = ebvo_grow(ctx, s, s.tq_i32, sizeof(int32_t) * (2 * nk1 + 2) + 16)))
        return rc;
    int32_t *cnt = (int32_t *)s.tq_i32.p, *rp = cnt + nk1;
    EBVO_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(int32_t) * 2 * nk1, s.stream));
    const ebvo_edge *cfL, *cfR;
    final_mates(s, &cfL, &cfR);
    const int cell = p->cell_size, gw = (int)(((int64_t)w + cell - 1) / cell), gh = (int)(((int64_t)h + cell - 1) / cell);
    // ceil(radius / cell) in double, saturated: the keyframe may come from a frame of another size, so the bound is not
    // gw + gh of this one but 2^30 cells, more than any distance between the cell of an edge of a frame the context holds
    // (at most 2^28 pixels) and a grid cell -- the saturated radius selects the same cells.  temporal_candidates_kernel
    // clips its walk to the grid, so a radius wider than the grid costs what the whole grid costs.
    const double sr_d = ceil(p->grid_radius / cell);
    const int sr = sr_d < (double)(1 << 30) ? (int)sr_d : (1 << 30);
    if ((rc = ebvo_grow(ctx, s, s.tq_cells, match_temporal_grid_bytes(n_cf, gw * gh))))
        return rc;
    void *grid = s.tq_cells.p;
    // under a pose prior (ebvo_temporal_set_prior) the projection comes first on the slot's stream, and both passes of the
    // walk take their query points from it
    TemporalPrior prior_q;
    const TemporalPrior *prior = nullptr;
    if (s.tq_prior.on)
    {
        if ((rc = temporal_prior_enqueue(ctx, s, &prior_q)))
            return rc;
        prior = &prior_q;
    }
    if ((rc = match_temporal_cells_enqueue(ctx, s, cfL, cfR, n_cf, cell, gw, gh, grid)) ||
        (rc = match_temporal_candidates_enqueue(ctx, s, ctx->kf_L, ctx->kf_R, n_kf, cfL, cfR, grid, n_cf, cell, sr, gw, gh,
                                                p->orient_thr_deg, cnt, nullptr, nullptr, 0, prior)) ||
        (rc = ebvo_device_scan(ctx, s, cnt, rp, n_kf, nullptr, 1, n_kf + 1)))
        return rc;
    if (size_first)
    {
        int32_t nq = 0;
        if ((rc = read_i32(ctx, s, rp + n_kf, &nq)))
            return rc;
        s.tq_cap = (int64_t)nq + nq / 4 + 1024;
    }
    const size_t capz = (size_t)s.tq_cap, ncz = (size_t)n_cf;
    if ((rc = ebvo_grow(ctx, s, s.tq_cols, sizeof(int32_t) * 2 * capz)) || (rc = ebvo_grow(ctx, s, s.tq_f64, sizeof(double) * 2 * capz)) ||
        (rc = ebvo_grow(ctx, s, s.tq_u8, 2 * ncz + capz + 64)) || (rc = ebvo_grow(ctx, s, s.patches_raw, sizeof(float) * 98 * ncz)) ||
        (rc = ebvo_grow(ctx, s, s.patches_norm, sizeof(float) * 98 * ncz)) || (rc = ebvo_grow(ctx, s, s.patches_flag, 2 * ncz)))
        return rc;
    int32_t *col = (int32_t *)s.tq_cols.p, *quad_kf = col + capz;
    double *sim_l = (double *)s.tq_f64.p, *sim_r = sim_l + capz;
    uint8_t *flagR = (uint8_t *)s.tq_u8.p, *keep = flagR + ((2 * ncz + 63) & ~(size_t)63);
    float *cfLn = (float *)s.patches_norm.p, *cfRn = (float *)s.patches_raw.p;
    uint8_t *cfLf = (uint8_t *)s.patches_flag.p;
    const int32_t *d_nq = rp + n_kf;
    if ((rc = match_temporal_candidates_enqueue(ctx, s, ctx->kf_L, ctx->kf_R, n_kf, cfL, cfR, grid, n_cf, cell, sr, gw, gh,
                                                p->orient_thr_deg, nullptr, rp, col, s.tq_cap, prior)) ||
        (rc = match_expand_rows_enqueue(ctx, s, rp, n_kf, s.tq_cap, quad_kf)) ||
        (rc = match_patches_enqueue(ctx, s, ncc_img(s, 0), h, w, w, cfL, n_cf, nullptr, 0, nullptr, cfLn, cfLf)) ||
        (rc = match_patches_enqueue(ctx, s, s.im[1].img, h, w, w, cfR, n_cf, nullptr, 0, nullptr, cfRn, flagR)) ||
        (rc = match_ncc_quads_indexed_enqueue(ctx, s, ctx->kf_Ln, ctx->kf_Lf, ctx->kf_Rn, ctx->kf_Rf, cfLn, cfLf, cfRn, flagR, quad_kf,
                                              col, s.tq_cap, p->ncc_thr, sim_l, sim_r, keep, d_nq)) ||
        (rc = match_count_flags_enqueue(ctx, s, keep, s.tq_cap, s.d_tq_tot + 1, d_nq)))
        return rc;
    // candidate count (an int32 of the row offsets) widened into the first word on the device side of the copy below
    EBVO_HIP(ctx, hipMemsetAsync(s.d_tq_tot, 0, sizeof(unsigned long long), s.stream));
    EBVO_HIP(ctx, hipMemcpyAsync(s.d_tq_tot, d_nq, sizeof(int32_t), hipMemcpyDeviceToDevice, s.stream)); // little-endian low word
    EBVO_HIP(ctx, hipMemcpyAsync(s.h_tq_tot, s.d_tq_tot, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipEventRecord(s.ev_tq, s.stream));
    return EBVO_OK;
}

extern "C" int ebvo_temporal_match_submit(ebvo_ctx *ctx, int slot, const ebvo_temporal_params *p)
{
    Slot *sp;
    if (!p || p->cell_size < 1 || !(p->grid_radius >= 0 && std::isfinite(p->grid_radius)) || !(p->orient_thr_deg >= 0) || (p->stages & ~1) ||
        (p->stages && (!(p->sift_thr > 0) || !(p->bnb_ncc >= 0) || !(p->bnb_sift >= 0) || p->gn.max_iter < 1 || !(p->gn.tol >= 0) ||
                       !(p->gn.huber_delta > 0))) ||
        get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_final || s.in_flight || s.fin_in_flight || s.tq_in_flight || ctx->kf_n < 0)
    {
        ctx->last_error = !s.have_final ? "the slot holds no final stereo mates (ebvo_stereo_finalize first)"
                          : ctx->kf_n < 0 ? "no keyframe (ebvo_temporal_set_keyframe first)"
                                          : "the slot has work in flight (wait for it first)";
        return EBVO_ERR_STATE;
    }
    if (p->stages && (s.cur_h != ctx->kf_h || s.cur_w != ctx->kf_w))
    {
        // the refinement of the quads samples the keyframe's images with the current frame's shape: refused before the slot's
        // earlier quads are dropped (stages = 0 reads stored patches only and works across sizes)
        ctx->last_error = "stages != 0 needs a current frame of the keyframe's size (the refinement samples both images with one shape)";
        return EBVO_ERR_STATE;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc_f = drain_fetch(ctx, s))
        return rc_f;
    s.tq_n = -1;
    s.tgt_armed = false; // the ground truth was given for the match that is replaced here
    s.tq_trail = Slot::TqTrail();
    s.tq_trail.on = s.tq_keep;
    s.tq_n_kf = ctx->kf_n;
    s.tq_kf_gen = ctx->kf_gen;
    s.tq_final = Slot::TqFinal();
    s.tq_params = *p;
    s.tq_empty = ctx->kf_n == 0 || s.n_final == 0;
    s.h_tq_tot[0] = s.h_tq_tot[1] = 0;
    // the pending prior becomes this match's; it stays pending until the submission has succeeded
    s.tq_prior = s.tq_prior_next;
    if (s.tq_empty)
    {
        // no quads at all: zeroed row offsets, nothing else to run (under a prior: the projection, for ebvo_temporal_prior_fetch)
        const size_t nk1 = (size_t)ctx->kf_n + 1;
        int rc = ebvo_grow(ctx, s, s.tq_i32, sizeof(int32_t) * (2 * nk1 + 2) + 16);
        if (rc)
            return rc;
        EBVO_HIP(ctx, hipMemsetAsync(s.tq_i32.p, 0, sizeof(int32_t) * 2 * nk1, s.stream));
        if (s.tq_prior.on)
        {
            const TemporalGridScope grid_scope(ctx, s);
            if ((rc = temporal_prior_enqueue(ctx, s, nullptr)))
            {
                (void)hipStreamSynchronize(s.stream);
                return rc;
            }
        }
        EBVO_HIP(ctx, hipEventRecord(s.ev_tq, s.stream));
        s.tq_in_flight = true;
        s.tq_prior_next.on = false;
        return EBVO_OK;
    }
    int rc = temporal_stage0_enqueue(ctx, s, p, s.tq_cap == 0);
    if (rc)
    {
        (void)hipStreamSynchronize(s.stream);
        return rc;
    }
    s.tq_in_flight = true;
    s.tq_prior_next.on = false;
    return EBVO_OK;
}

// the chain did not run (no quads at all): every interior stage of a kept trail is an empty list over the zeroed offsets
static void trail_all_empty(Slot &s, const int32_t *zero_rp)
{
    if (!s.tq_trail.on)
        return;
    for (int k = 0; k < 4; ++k)
    {
        s.tq_trail.rp[k] = zero_rp;
        s.tq_trail.cf[k] = nullptr;
        s.tq_trail.n[k] = 0;
    }
    s.tq_trail.lists = true;
}

extern "C" int ebvo_temporal_keep_stages(ebvo_ctx *ctx, int slot, int on)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    if (sp->tq_in_flight)
    {
        ctx->last_error = "a temporal match is in flight in the slot (ebvo_temporal_match_wait first)";
        return EBVO_ERR_STATE;
    }
    sp->tq_keep = on != 0; // read by the next ebvo_temporal_match_submit; the slot's match and armed state stay
    return EBVO_OK;
}

extern "C" int ebvo_temporal_match_wait(ebvo_ctx *ctx, int slot, ebvo_temporal_counts *counts)
{
    Slot *sp;
    if (!counts || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.tq_in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    s.tq_in_flight = false;
    memset(counts, 0, sizeof *counts);
    const ebvo_temporal_params &P = s.tq_params;
    const int n_kf = s.tq_n_kf, n_cf = s.n_final;
    counts->n_kf = n_kf;
    counts->n_cf = n_cf;
    EBVO_HIP(ctx, hipEventSynchronize(s.ev_tq));
    if (s.tq_kf_gen != ctx->kf_gen)
    {
        // second line of defence (ebvo_temporal_set_keyframe refuses while a match is in flight): the lists were formed against
        // a keyframe that is gone, and the chain below would read the new one's descriptors and images with them
        ctx->last_error = "the keyframe was replaced while the match was in flight";
        return EBVO_ERR_STATE;
    }
    const size_t nk1 = (size_t)n_kf + 1;
    int32_t *rp = (int32_t *)s.tq_i32.p + nk1;
    if (s.tq_empty)
    {
        s.tq_n = 0;
        if (P.stages)
        {
            s.tq_final.rp = rp;
            s.tq_final.n = 0;
            trail_all_empty(s, rp);
        }
        return EBVO_OK;
    }
    int64_t nq = (int64_t)s.h_tq_tot[0];
    if (nq > s.tq_cap)
    {
        // more candidate quads than the buffers were sized for: size them for this frame and run the stages again
        s.tq_cap = 0;
        int rc = temporal_stage0_enqueue(ctx, s, &P, true);
        if (rc)
        {
            (void)hipStreamSynchronize(s.stream);
            return rc;
        }
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_tq));
        nq = (int64_t)s.h_tq_tot[0];
    }
    const int64_t kept = (int64_t)s.h_tq_tot[1];
    counts->n_candidates = nq;
    counts->n_kept = kept;
    s.tq_n = nq;
    s.tq_final.n = -1;
    if (nq == 0)
    {
        if (P.stages)
        {
            s.tq_final.rp = rp; // the scanned counts: all zero
            s.tq_final.n = 0;
            trail_all_empty(s, rp);
        }
        return EBVO_OK;
    }
    if (P.stages == 0)
        return EBVO_OK;
    const size_t capz = (size_t)s.tq_cap, ncz = (size_t)n_cf;
    const ebvo_edge *cfL, *cfR;
    final_mates(s, &cfL, &cfR);
    const int32_t *col = (const int32_t *)s.tq_cols.p, *quad_kf = col + capz;
    const double *sim_l = (const double *)s.tq_f64.p;
    const uint8_t *keep = (const uint8_t *)s.tq_u8.p + ((2 * ncz + 63) & ~(size_t)63);
    return temporal_chain(ctx, s, P, rp, col, quad_kf, sim_l, keep, n_kf, cfL, cfR, n_cf, kept, counts);
}

extern "C" int ebvo_temporal_match(ebvo_ctx *ctx, int slot, const ebvo_temporal_params *p, ebvo_temporal_counts *counts)
{
    if (!counts)
        return EBVO_ERR_ARG;
    int rc = ebvo_temporal_match_submit(ctx, slot, p);
    return rc ? rc : ebvo_temporal_match_wait(ctx, slot, counts);
}

extern "C" int ebvo_temporal_fetch_final(ebvo_ctx *ctx, int slot, int32_t *row_ptr, int32_t *cf_index, ebvo_edge *left,
                                         ebvo_edge *right, double *ncc_left, double *sift_left, double *score_left,
                                         double *score_right, uint8_t *valid)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.tq_final.n < 0 || s.in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const Slot::TqFinal &F = s.tq_final;
    const size_t nk1 = (size_t)s.tq_n_kf + 1, n = (size_t)F.n;
    hipStream_t st = s.stream;
    if (row_ptr)
        EBVO_HIP(ctx, hipMemcpyAsync(row_ptr, F.rp, sizeof(int32_t) * nk1, hipMemcpyDeviceToHost, st));
    if (n)
    {
        const struct
        {
            void *dst;
            const void *src;
            size_t bytes;
        } copies[] = {{cf_index, F.cf, sizeof(int32_t) * n}, {left, F.L, sizeof(ebvo_edge) * n}, {right, F.R, sizeof(ebvo_edge) * n},
                      {ncc_left, F.ncc, sizeof(double) * n}, {sift_left, F.sift, sizeof(double) * n},
                      {score_left, F.sL, sizeof(double) * n}, {score_right, F.sR, sizeof(double) * n}, {valid, F.valid, n}};
        for (const auto &c : copies)
            if (c.dst)
                EBVO_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, st));
    }
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    return EBVO_OK;
}

extern "C" int ebvo_temporal_fetch(ebvo_ctx *ctx, int slot, int32_t *row_ptr, int32_t *col_idx, double *sim_left, double *sim_right,
                                   uint8_t *keep)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.tq_n < 0 || s.in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nk1 = (size_t)s.tq_n_kf + 1, nq = (size_t)s.tq_n, ncz = (size_t)s.n_final, capz = (size_t)s.tq_cap;
    hipStream_t st = s.stream;
    if (row_ptr)
        EBVO_HIP(ctx, hipMemcpyAsync(row_ptr, (const int32_t *)s.tq_i32.p + nk1, sizeof(int32_t) * nk1, hipMemcpyDeviceToHost, st));
    if (nq)
    {
        if (col_idx)
            EBVO_HIP(ctx, hipMemcpyAsync(col_idx, s.tq_cols.p, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
        if (sim_left)
            EBVO_HIP(ctx, hipMemcpyAsync(sim_left, s.tq_f64.p, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
        if (sim_right)
            EBVO_HIP(ctx, hipMemcpyAsync(sim_right, (const double *)s.tq_f64.p + capz, sizeof(double) * nq, hipMemcpyDeviceToHost, st));
        if (keep)
            EBVO_HIP(ctx, hipMemcpyAsync(keep, (const uint8_t *)s.tq_u8.p + ((2 * ncz + 63) & ~(size_t)63), nq, hipMemcpyDeviceToHost, st));
    }
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    return EBVO_OK;
}

// ---- relative pose from the temporal quads (pose_kernels.hip) ----------------------------------------------------------
extern "C" void ebvo_pose_default_params(ebvo_pose_params *p)
{
    if (!p)
        return;
    p->max_iterations = 5000; // Ransac_Options (include/MotionTracker.h)
    p->min_iterations = 1000;
    p->dyn_num_trials_mult = 3.0;
    p->success_prob = 0.97;
    p->max_reproj_error = 1.5;
    p->top_rank_fraction = 0.7;
    p->tau_length = 0.13; // TAU_C1..C4 (include/definitions.h)
    p->tau_t1 = 0.12;
    p->tau_t2 = 0.12;
    p->tau_tangent = 0.32;
    p->rand_seed = 1;
    p->continue_stream = 0;
    p->max_draws = (int64_t)1 << 22;
}

static bool pose_args_ok(const ebvo_stereo_calib *cal, const ebvo_pose_params *p, const ebvo_pose_result *res)
{
    if (!cal || !p || !res)
        return false;
    for (int i = 0; i < 9; ++i)
        if (std::isnan(cal->K_left[i]) || std::isnan(cal->R21[i]))
            return false;
    for (int i = 0; i < 3; ++i)
        if (std::isnan(cal->T21[i]))
            return false;
    const double tau[] = {p->max_reproj_error, p->tau_length, p->tau_t1, p->tau_t2, p->tau_tangent};
    for (double v : tau)
        if (!(v >= 0)) // NaN or negative; +inf is allowed
            return false;
    return p->success_prob > 0 && p->success_prob < 1 && p->top_rank_fraction > 0 && p->top_rank_fraction <= 1 &&
           p->max_iterations >= 0 && p->min_iterations >= 0 && p->max_draws >= 1 && p->dyn_num_trials_mult > 0;
}

extern "C" int ebvo_temporal_final_size(ebvo_ctx *ctx, int slot, int32_t *n_kf, int64_t *n_final)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp) || !n_kf || !n_final)
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.tq_final.n < 0 || s.in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    *n_kf = s.tq_n_kf;
    *n_final = s.tq_final.n;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_estimate_pose(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
                                           ebvo_pose_result *res, uint8_t *inlier)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp) || !pose_args_ok(cal, p, res))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.tq_final.n < 0 || s.in_flight || s.fin_in_flight || s.tq_in_flight || s.tq_kf_gen != ctx->kf_gen)
    {
        ctx->last_error = s.tq_final.n < 0 ? "the slot holds no final quads (ebvo_temporal_match with stages = 1 first)"
                          : s.tq_kf_gen != ctx->kf_gen ? "the keyframe was replaced since the slot's quads were matched"
                                                       : "the slot has work in flight (wait for it first)";
        return EBVO_ERR_STATE;
    }
    if (s.tq_final.n > INT32_MAX)
        return EBVO_ERR_ARG;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const Slot::TqFinal &F = s.tq_final;
    return pose_run(ctx, s, ctx->kf_L, ctx->kf_R, F.rp, s.tq_n_kf, F.L, F.R, (int)F.n, cal, p, res, inlier, nullptr, nullptr);
}

extern "C" int ebvo_pose_from_quads(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf,
                                    const int32_t *row_ptr, const ebvo_edge *cf_left, const ebvo_edge *cf_right,
                                    const ebvo_stereo_calib *cal, const ebvo_pose_params *p, ebvo_pose_result *res,
                                    uint8_t *inlier, double *quad_geom, int32_t *rank_order)
{
    int64_t np = 0;
    if (!ctx || (n_kf > 0 && (!kf_left || !kf_right)) || !pose_args_ok(cal, p, res) || check_csr(row_ptr, n_kf, &np))
        return EBVO_ERR_ARG;
    const int n = (int)np;
    if (n > 0 && (!cf_left || !cf_right))
        return EBVO_ERR_ARG;
    Slot &s = *ctx->slots[0];
    if (s.in_flight || s.fin_in_flight || s.tq_in_flight)
    {
        ctx->last_error = "slot 0 has submitted work in flight; wait for it first";
        return EBVO_ERR_STATE;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (n < 2 || (int64_t)(p->top_rank_fraction * (double)n) < 2) // insufficient: nothing to upload or launch
        return pose_run(ctx, s, nullptr, nullptr, nullptr, n_kf, nullptr, nullptr, n, cal, p, res, inlier, nullptr, nullptr);
    // uploaded into the slot's own pose buffer: the slot's resident results stay as they are
    const size_t ek = sizeof(ebvo_edge) * (size_t)n_kf, eq = sizeof(ebvo_edge) * (size_t)n, rb = sizeof(int32_t) * ((size_t)n_kf + 1);
    int rc;
    if ((rc = ebvo_grow(ctx, s, s.pose_in, 2 * ek + 2 * eq + rb)))
        return rc;
    uint8_t *base = (uint8_t *)s.pose_in.p;
    ebvo_edge *d_kfL = (ebvo_edge *)base, *d_kfR = (ebvo_edge *)(base + ek), *d_cfL = (ebvo_edge *)(base + 2 * ek),
              *d_cfR = (ebvo_edge *)(base + 2 * ek + eq);
    int32_t *d_rp = (int32_t *)(base + 2 * ek + 2 * eq);
    hipStream_t st = s.stream;
    EBVO_HIP(ctx, hipMemcpyAsync(d_kfL, kf_left, ek, hipMemcpyHostToDevice, st));
    EBVO_HIP(ctx, hipMemcpyAsync(d_kfR, kf_right, ek, hipMemcpyHostToDevice, st));
    EBVO_HIP(ctx, hipMemcpyAsync(d_cfL, cf_left, eq, hipMemcpyHostToDevice, st));
    EBVO_HIP(ctx, hipMemcpyAsync(d_cfR, cf_right, eq, hipMemcpyHostToDevice, st));
    EBVO_HIP(ctx, hipMemcpyAsync(d_rp, row_ptr, rb, hipMemcpyHostToDevice, st));
    return pose_run(ctx, s, d_kfL, d_kfR, d_rp, n_kf, d_cfL, d_cfR, n, cal, p, res, inlier, quad_geom, rank_order);
}

// ---- the pose stage under ground truth (pose_kernels.hip: row selection, constraint cascade) --------------------------
static bool pose_cascade_args_ok(const ebvo_pose_params *p, int n_runs, const ebvo_pose_cascade_run *runs)
{
    return runs && n_runs >= 1 && (int64_t)n_runs * (int64_t)p->max_iterations <= ((int64_t)1 << 24);
}

// Host quads of a GT call, checked, counted and uploaded into slot 0's own pose buffer.  n_listed / n_sel: listed rows and
// selected quads, counted here; upload = false: only check and count.
struct PoseHostQuads
{
    const ebvo_edge *kfL = nullptr, *kfR = nullptr, *cfL = nullptr, *cfR = nullptr;
    const int32_t *rp = nullptr;
    const uint8_t *on = nullptr, *tp = nullptr;
    int n = 0;
    int64_t n_listed = 0, n_sel = 0;
};

static int pose_host_quads_check(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const int32_t *row_ptr,
                                 const ebvo_edge *cf_left, const ebvo_edge *cf_right, const uint8_t *row_listed, const uint8_t *kf_is_tp,
                                 PoseHostQuads *q)
{
    int64_t np = 0;
    if (!ctx || (n_kf > 0 && (!kf_left || !kf_right)) || check_csr(row_ptr, n_kf, &np))
        return EBVO_ERR_ARG;
    q->n = (int)np;
    if (q->n > 0 && (!cf_left || !cf_right))
        return EBVO_ERR_ARG;
    q->n_listed = q->n_sel = 0;
    for (int i = 0; i < n_kf; ++i)
    {
        const bool listed = !row_listed || row_listed[i];
        q->n_listed += listed;
        if (listed && (!kf_is_tp || kf_is_tp[i]))
            q->n_sel += row_ptr[i + 1] - row_ptr[i];
    }
    Slot &s = *ctx->slots[0];
    if (s.in_flight || s.fin_in_flight || s.tq_in_flight)
    {
        ctx->last_error = "slot 0 has submitted work in flight; wait for it first";
        return EBVO_ERR_STATE;
    }
    return EBVO_OK;
}

static int pose_host_quads_upload(ebvo_ctx *ctx, Slot &s, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf,
                                  const int32_t *row_ptr, const ebvo_edge *cf_left, const ebvo_edge *cf_right, const uint8_t *row_listed,
                                  const uint8_t *kf_is_tp, const uint8_t *quad_is_tp, PoseHostQuads *q)
{
    const size_t kz = (size_t)n_kf, nz = (size_t)q->n;
    const size_t ek = sizeof(ebvo_edge) * kz, eq = sizeof(ebvo_edge) * nz, rb = sizeof(int32_t) * (kz + 1);
    Carve L;
    const size_t o_kfL = L.take(ek), o_kfR = L.take(ek), o_cfL = L.take(eq), o_cfR = L.take(eq), o_rp = L.take(rb), o_on = L.take(kz),
                 o_tp = L.take(nz);
    int rc = ebvo_grow(ctx, s, s.pose_in, L.total());
    if (rc)
        return rc;
    char *base = (char *)s.pose_in.p;
    q->kfL = (ebvo_edge *)(base + o_kfL);
    q->kfR = (ebvo_edge *)(base + o_kfR);
    q->cfL = (ebvo_edge *)(base + o_cfL);
    q->cfR = (ebvo_edge *)(base + o_cfR);
    q->rp = (int32_t *)(base + o_rp);
    q->on = (uint8_t *)(base + o_on);
    q->tp = quad_is_tp ? (uint8_t *)(base + o_tp) : nullptr;
    std::vector<uint8_t> on(kz);
    for (size_t i = 0; i < kz; ++i)
        on[i] = (!row_listed || row_listed[i]) && (!kf_is_tp || kf_is_tp[i]);
    hipStream_t st = s.stream;
    (rc = copy_up(ctx, st, base + o_kfL, kf_left, ek)) || (rc = copy_up(ctx, st, base + o_kfR, kf_right, ek)) ||
        (rc = copy_up(ctx, st, base + o_cfL, cf_left, eq)) || (rc = copy_up(ctx, st, base + o_cfR, cf_right, eq)) ||
        (rc = copy_up(ctx, st, base + o_rp, row_ptr, rb)) || (rc = copy_up(ctx, st, base + o_on, on.data(), kz)) ||
        (rc = copy_up(ctx, st, base + o_tp, quad_is_tp, nz));
    // `on` is a local and the other sources are the caller's; the pose kernels read the buffer after this returns
    const hipError_t e = hipStreamSynchronize(st);
    if (rc)
        return rc;
    EBVO_HIP(ctx, e);
    return EBVO_OK;
}

static bool pose_gt_insufficient(const PoseHostQuads &q, const ebvo_pose_params *p)
{
    return q.n_listed < 2 || q.n_sel < 2 || (int64_t)(p->top_rank_fraction * (double)q.n_sel) < 2;
}

extern "C" int ebvo_pose_from_quads_gt(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf,
                                       const int32_t *row_ptr, const ebvo_edge *cf_left, const ebvo_edge *cf_right,
                                       const uint8_t *row_listed, const uint8_t *kf_is_tp, const ebvo_stereo_calib *cal,
                                       const ebvo_pose_params *p, ebvo_pose_result *res, uint8_t *inlier, double *quad_geom,
                                       int32_t *rank_order)
{
    if (!ctx || !pose_args_ok(cal, p, res))
        return EBVO_ERR_ARG;
    PoseHostQuads q;
    if (int rc = pose_host_quads_check(ctx, kf_left, kf_right, n_kf, row_ptr, cf_left, cf_right, row_listed, kf_is_tp, &q))
        return rc;
    Slot &s = *ctx->slots[0];
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (pose_gt_insufficient(q, p)) // nothing to upload or launch
    {
        if (int rc = pose_run(ctx, s, nullptr, nullptr, nullptr, 0, nullptr, nullptr, (int)q.n_sel, cal, p, res, nullptr, nullptr, nullptr,
                              true))
            return rc;
        if (inlier && q.n > 0)
            memset(inlier, 0, (size_t)q.n);
        return EBVO_OK;
    }
    if (int rc = pose_host_quads_upload(ctx, s, kf_left, kf_right, n_kf, row_ptr, cf_left, cf_right, row_listed, kf_is_tp, nullptr, &q))
        return rc;
    return pose_run_gt(ctx, s, q.kfL, q.kfR, q.rp, n_kf, q.cfL, q.cfR, q.n, q.on, q.n_listed, cal, p, res, inlier, quad_geom, rank_order);
}

extern "C" int ebvo_pose_constraint_metrics(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf,
                                            const int32_t *row_ptr, const ebvo_edge *cf_left, const ebvo_edge *cf_right,
                                            const uint8_t *row_listed, const uint8_t *kf_is_tp, const uint8_t *quad_is_tp,
                                            const ebvo_stereo_calib *cal, const ebvo_pose_params *p, int n_runs,
                                            ebvo_pose_cascade_run *runs, int32_t *draw_idx, uint8_t *draw_stage)
{
    ebvo_pose_result unused;
    if (!ctx || !pose_args_ok(cal, p, &unused) || !pose_cascade_args_ok(p, n_runs, runs))
        return EBVO_ERR_ARG;
    PoseHostQuads q;
    if (int rc = pose_host_quads_check(ctx, kf_left, kf_right, n_kf, row_ptr, cf_left, cf_right, row_listed, kf_is_tp, &q))
        return rc;
    Slot &s = *ctx->slots[0];
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (pose_gt_insufficient(q, p))
    {
        pose_cascade_insufficient(ctx, p, q.n_sel, n_runs, runs);
        return EBVO_OK;
    }
    if (int rc = pose_host_quads_upload(ctx, s, kf_left, kf_right, n_kf, row_ptr, cf_left, cf_right, row_listed, kf_is_tp, quad_is_tp, &q))
        return rc;
    return pose_cascade_run(ctx, s, q.kfL, q.kfR, q.rp, n_kf, q.cfL, q.cfR, q.n, q.on, q.n_listed, q.tp, cal, p, n_runs, runs, draw_idx,
                            draw_stage);
}

static int tgt_armed_slot(ebvo_ctx *ctx, int slot, Slot **out);

// the armed slot of the resident GT pose calls: its match formed the final quads
static int pose_gt_slot(ebvo_ctx *ctx, int slot, Slot **out)
{
    if (int rc = tgt_armed_slot(ctx, slot, out))
        return rc;
    if ((*out)->tq_final.n < 0)
    {
        ctx->last_error = "the slot holds no final quads (ebvo_temporal_match with stages = 1, then ebvo_temporal_set_gt)";
        return EBVO_ERR_STATE;
    }
    return (*out)->tq_final.n > INT32_MAX ? EBVO_ERR_ARG : EBVO_OK;
}

extern "C" int ebvo_temporal_estimate_pose_gt(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
                                              ebvo_pose_result *res, uint8_t *inlier)
{
    if (!ctx || !pose_args_ok(cal, p, res))
        return EBVO_ERR_ARG;
    Slot *sp;
    if (int rc = pose_gt_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const Slot::TqFinal &F = s.tq_final;
    const uint8_t *on = (const uint8_t *)s.tgt_u8.p + (size_t)s.tgt_n_kf; // row_on[]: a veridical quad and kf_is_tp
    return pose_run_gt(ctx, s, ctx->kf_L, ctx->kf_R, F.rp, s.tq_n_kf, F.L, F.R, (int)F.n, on, s.tgt_n_rows, cal, p, res, inlier, nullptr,
                       nullptr);
}

extern "C" int ebvo_temporal_pose_constraint_metrics(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
                                                     int n_runs, ebvo_pose_cascade_run *runs, int32_t *draw_idx, uint8_t *draw_stage)
{
    ebvo_pose_result unused;
    if (!ctx || !pose_args_ok(cal, p, &unused) || !pose_cascade_args_ok(p, n_runs, runs))
        return EBVO_ERR_ARG;
    Slot *sp;
    if (int rc = pose_gt_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const Slot::TqFinal &F = s.tq_final;
    const uint8_t *on = (const uint8_t *)s.tgt_u8.p + (size_t)s.tgt_n_kf;
    // the EBVO_TGT_CLUSTER flags of ebvo_temporal_gt_flags; no row is on when arming walked nothing, so they are not read then
    const uint8_t *tp = (const uint8_t *)s.tgt_flags.p + 2 * (size_t)s.tq_n;
    return pose_cascade_run(ctx, s, ctx->kf_L, ctx->kf_R, F.rp, s.tq_n_kf, F.L, F.R, (int)F.n, on, s.tgt_n_rows, tp, cal, p, n_runs, runs,
                            draw_idx, draw_stage);
}

// ---- inlier refit of the relative pose (pose_refit_kernels.hip) ----------------------------------------------------------
extern "C" void ebvo_pose_refine_default_params(ebvo_pose_refine_params *p)
{
    if (!p)
        return;
    p->rounds = 2;
    p->iterations = 10;
    p->huber_px = 1.5;
    p->step_eps = 1e-10;
    p->block_threads = 0;
    p->reserved = 0;
}

static bool pose_refine_args_ok(const ebvo_pose_refine_params *rp, const double *R0, const double *t0, const ebvo_pose_refined *out)
{
    if (!rp || !R0 || !t0 || !out)
        return false;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R0[i]))
            return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(t0[i]))
            return false;
    const int bt = rp->block_threads;
    return rp->rounds >= 1 && rp->rounds <= 16 && rp->iterations >= 0 && rp->iterations <= 100 && rp->huber_px > 0 && rp->step_eps >= 0 &&
           (bt == 0 || bt == 256 || bt == 512 || bt == 1024);
}

extern "C" int ebvo_pose_refine_from_quads(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf,
                                           const int32_t *row_ptr, const ebvo_edge *cf_left, const ebvo_edge *cf_right,
                                           const uint8_t *row_listed, const uint8_t *kf_is_tp, const ebvo_stereo_calib *cal,
                                           const ebvo_pose_params *p, const ebvo_pose_refine_params *rp, const double R0[9],
                                           const double t0[3], ebvo_pose_refined *out, uint8_t *inlier)
{
    ebvo_pose_result unused;
    if (!ctx || !pose_args_ok(cal, p, &unused) || !pose_refine_args_ok(rp, R0, t0, out))
        return EBVO_ERR_ARG;
    PoseHostQuads q;
    if (int rc = pose_host_quads_check(ctx, kf_left, kf_right, n_kf, row_ptr, cf_left, cf_right, row_listed, kf_is_tp, &q))
        return rc;
    Slot &s = *ctx->slots[0];
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (q.n_sel < 2) // nothing to upload or launch
    {
        memset(out, 0, sizeof *out);
        memcpy(out->R, R0, sizeof out->R);
        memcpy(out->t, t0, sizeof out->t);
        out->status = 1;
        out->stop_reason = 4;
        out->n_quads = q.n_sel;
        if (inlier && q.n > 0)
            memset(inlier, 0, (size_t)q.n);
        return EBVO_OK;
    }
    if (int rc = pose_host_quads_upload(ctx, s, kf_left, kf_right, n_kf, row_ptr, cf_left, cf_right, row_listed, kf_is_tp, nullptr, &q))
        return rc;
    return pose_refit_run(ctx, s, q.kfL, q.kfR, q.rp, n_kf, q.cfL, q.cfR, q.n, row_listed || kf_is_tp ? q.on : nullptr, cal, p, rp, R0, t0,
                          out, inlier);
}

extern "C" int ebvo_temporal_refine_pose(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
                                         const ebvo_pose_refine_params *rp, const double R0[9], const double t0[3], int gt_rows,
                                         ebvo_pose_refined *out, uint8_t *inlier)
{
    ebvo_pose_result unused;
    Slot *sp;
    if (!ctx || !pose_args_ok(cal, p, &unused) || !pose_refine_args_ok(rp, R0, t0, out) || (gt_rows != 0 && gt_rows != 1))
        return EBVO_ERR_ARG;
    if (gt_rows)
    {
        if (int rc = pose_gt_slot(ctx, slot, &sp))
            return rc;
    }
    else
    {
        if (get_slot(ctx, slot, &sp))
            return EBVO_ERR_ARG;
        Slot &s = *sp;
        if (s.tq_final.n < 0 || s.in_flight || s.fin_in_flight || s.tq_in_flight || s.tq_kf_gen != ctx->kf_gen)
        {
            ctx->last_error = s.tq_final.n < 0 ? "the slot holds no final quads (ebvo_temporal_match with stages = 1 first)"
                              : s.tq_kf_gen != ctx->kf_gen ? "the keyframe was replaced since the slot's quads were matched"
                                                           : "the slot has work in flight (wait for it first)";
            return EBVO_ERR_STATE;
        }
        if (s.tq_final.n > INT32_MAX)
            return EBVO_ERR_ARG;
    }
    Slot &s = *sp;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const Slot::TqFinal &F = s.tq_final;
    const uint8_t *on = gt_rows ? (const uint8_t *)s.tgt_u8.p + (size_t)s.tgt_n_kf : nullptr; // row_on[], as the GT search
    return pose_refit_run(ctx, s, ctx->kf_L, ctx->kf_R, F.rp, s.tq_n_kf, F.L, F.R, (int)F.n, on, cal, p, rp, R0, t0, out, inlier);
}

// ---- alignment of the pose to the current frame's TOED edges (align_kernels.hip) ---------------------------------------
extern "C" void ebvo_align_default_params(ebvo_align_params *p)
{
    if (!p)
        return;
    p->rounds = 4;
    p->iterations = 10;
    p->radius = 4.0;
    p->cell_size = 4;
    p->min_terms = 12;
    p->orient_thr_deg = 10.0;
    p->huber_px = 1.0;
    p->inlier_px = 1.0;
    p->step_eps = 1e-10;
    p->img_margin = 10.0;
    p->cameras = 2;
    p->block_threads = 0;
}

static bool align_args_ok(const ebvo_stereo_calib *cal, const ebvo_align_params *ap, const double *R0, const double *t0,
                          const ebvo_aligned_pose *out, int img_w, int img_h)
{
    if (!cal || !ap || !R0 || !t0 || !out || img_w < 1 || img_h < 1)
        return false;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R0[i]))
            return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(t0[i]))
            return false;
    const int bt = ap->block_threads;
    // every comparison is false for a NaN
    if (!(ap->rounds >= 1 && ap->rounds <= 16 && ap->iterations >= 0 && ap->iterations <= 100 && std::isfinite(ap->radius) &&
          ap->radius > 0 && ap->cell_size >= 1 && ap->orient_thr_deg >= 0 && ap->huber_px > 0 && ap->inlier_px >= 0 &&
          ap->step_eps >= 0 && ap->min_terms >= 6 && ap->img_margin >= 0 && (ap->cameras == 1 || ap->cameras == 2) &&
          (bt == 0 || bt == 256 || bt == 512 || bt == 1024)))
        return false;
    if (!(ceil(ap->radius / ap->cell_size) <= 8.0))
        return false;
    const int64_t gw = ((int64_t)img_w + ap->cell_size - 1) / ap->cell_size, gh = ((int64_t)img_h + ap->cell_size - 1) / ap->cell_size;
    return gw * gh <= (1 << 26);
}

// nothing to launch: the start pose, status 1
static void align_nothing(const double *R0, const double *t0, int n_kf, ebvo_aligned_pose *out, int32_t *assoc_left, int32_t *assoc_right)
{
    memset(out, 0, sizeof *out);
    memcpy(out->R, R0, sizeof out->R);
    memcpy(out->t, t0, sizeof out->t);
    out->status = 1;
    out->stop_reason = 4;
    out->n_kf = n_kf;
    for (int i = 0; i < n_kf; ++i)
    {
        if (assoc_left)
            assoc_left[i] = -1;
        if (assoc_right)
            assoc_right[i] = -1;
    }
}

static void align_publish(const AlignResult &r, int n_kf, ebvo_aligned_pose *out)
{
    memset(out, 0, sizeof *out);
    memcpy(out->R, r.Rt, sizeof out->R);
    memcpy(out->t, r.Rt + 9, sizeof out->t);
    out->status = r.status;
    out->stop_reason = r.stop;
    out->rounds_run = r.rounds_run;
    out->steps_kept = r.steps_kept;
    out->n_kf = n_kf;
    out->fit_terms = r.fit_terms;
    out->n_assoc[0] = r.n_assoc[0];
    out->n_assoc[1] = r.n_assoc[1];
    out->inliers = r.inliers;
    out->cost_first = r.cost_first;
    out->cost_last = r.cost_last;
    out->rms_normal = r.rms_normal;
}

// lambda (host, may be NULL): the inverse-depth ratio per mate (ebvo_pose_align_edges_depth)
static int align_edges_host(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, const double *lambda, int n_kf,
                            const ebvo_edge *cf_edges_left, int n0, const ebvo_edge *cf_edges_right, int n1, int img_w, int img_h,
                            const ebvo_stereo_calib *cal, const ebvo_align_params *params, const double *R0, const double *t0,
                            ebvo_aligned_pose *out, int32_t *assoc_left, int32_t *assoc_right)
{
    if (!ctx || !align_args_ok(cal, params, R0, t0, out, img_w, img_h) || n_kf < 0 || n0 < 0 || (n_kf > 0 && (!kf_left || !kf_right)) ||
        (n0 > 0 && !cf_edges_left))
        return EBVO_ERR_ARG;
    if (params->cameras == 1)
        n1 = 0;
    else if (n1 < 0 || (n1 > 0 && !cf_edges_right))
        return EBVO_ERR_ARG;
    AlignResult r;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    if (n_kf == 0 || n0 + (int64_t)n1 == 0)
    {
        align_nothing(R0, t0, n_kf, out, assoc_left, assoc_right);
        return EBVO_OK;
    }
    const size_t nz = (size_t)n_kf, eb = sizeof(ebvo_edge);
    Carve L;
    const size_t o_kfL = L.take(eb * nz), o_kfR = L.take(eb * nz), o_E0 = L.take(eb * (size_t)n0), o_E1 = L.take(eb * (size_t)n1),
                 o_lam = L.take(lambda ? 8 * nz : 0);
    if (hc.stage(L))
        return hc.rc;
    ebvo_edge *kfL = hc.at<ebvo_edge>(o_kfL), *kfR = hc.at<ebvo_edge>(o_kfR), *E0 = hc.at<ebvo_edge>(o_E0), *E1 = hc.at<ebvo_edge>(o_E1);
    double *d_lam = lambda ? hc.at<double>(o_lam) : nullptr;
    if (hc.up(kfL, kf_left, eb * nz) || hc.up(kfR, kf_right, eb * nz) || hc.up(E0, cf_edges_left, eb * (size_t)n0) ||
        hc.up(E1, cf_edges_right, eb * (size_t)n1) || hc.up(d_lam, lambda, 8 * nz))
        return hc.rc;
    {
        const TemporalGridScope grid_scope(ctx, hc.slot());
        if (int rc = align_run(ctx, hc.slot(), kfL, kfR, n_kf, E0, n0, E1, n1, img_w, img_h, cal, params, R0, t0, d_lam, &r, assoc_left,
                               assoc_right))
            return rc;
    }
    if (hc.finish())
        return hc.rc;
    align_publish(r, n_kf, out);
    return EBVO_OK;
}

extern "C" int ebvo_pose_align_edges(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf,
                                     const ebvo_edge *cf_edges_left, int n0, const ebvo_edge *cf_edges_right, int n1, int img_w,
                                     int img_h, const ebvo_stereo_calib *cal, const ebvo_align_params *params, const double R0[9],
                                     const double t0[3], ebvo_aligned_pose *out, int32_t *assoc_left, int32_t *assoc_right)
{
    return align_edges_host(ctx, kf_left, kf_right, nullptr, n_kf, cf_edges_left, n0, cf_edges_right, n1, img_w, img_h, cal, params, R0, t0,
                            out, assoc_left, assoc_right);
}

extern "C" int ebvo_pose_align_edges_depth(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, const double *lambda,
                                           int n_kf, const ebvo_edge *cf_edges_left, int n0, const ebvo_edge *cf_edges_right, int n1,
                                           int img_w, int img_h, const ebvo_stereo_calib *cal, const ebvo_align_params *params,
                                           const double R0[9], const double t0[3], ebvo_aligned_pose *out, int32_t *assoc_left,
                                           int32_t *assoc_right)
{
    return align_edges_host(ctx, kf_left, kf_right, lambda, n_kf, cf_edges_left, n0, cf_edges_right, n1, img_w, img_h, cal, params, R0, t0,
                            out, assoc_left, assoc_right);
}

// a keyframe, and a pair on the slot whose wait has returned, nothing of the slot in flight
static int align_slot_state(ebvo_ctx *ctx, const Slot &s)
{
    if (ctx->kf_n < 0 || !s.have_run || s.in_flight || s.fin_in_flight || s.tq_in_flight)
    {
        ctx->last_error = s.in_flight || s.fin_in_flight || s.tq_in_flight ? "the slot has work in flight (wait for it first)"
                          : ctx->kf_n < 0                                  ? "no keyframe (ebvo_temporal_set_keyframe first)"
                                                                           : "the slot holds no pair (ebvo_stereo_submit and ebvo_stereo_wait first)";
        return EBVO_ERR_STATE;
    }
    return EBVO_OK;
}

extern "C" int ebvo_temporal_align_size(ebvo_ctx *ctx, int slot, int32_t *n_kf, int32_t *n_left, int32_t *n_right)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp) || !n_kf || !n_left || !n_right)
        return EBVO_ERR_ARG;
    if (int rc = align_slot_state(ctx, *sp))
        return rc;
    *n_kf = ctx->kf_n;
    *n_left = sp->im[0].n_kept;
    *n_right = sp->im[1].n_kept;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_align_pose(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_align_params *params,
                                        const double R0[9], const double t0[3], ebvo_aligned_pose *out, int32_t *assoc_left,
                                        int32_t *assoc_right)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    // the frame's size enters the accepted ranges through the grid; a slot without a pair has none yet
    if (!align_args_ok(cal, params, R0, t0, out, s.have_run ? s.cur_w : 1, s.have_run ? s.cur_h : 1))
        return EBVO_ERR_ARG;
    if (int rc = align_slot_state(ctx, s))
        return rc;
    const int n_kf = ctx->kf_n, n0 = s.im[0].n_kept, n1 = params->cameras > 1 ? s.im[1].n_kept : 0;
    if (n_kf == 0 || n0 + (int64_t)n1 == 0)
    {
        align_nothing(R0, t0, n_kf, out, assoc_left, assoc_right);
        return EBVO_OK;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    AlignResult r;
    int rc;
    {
        const TemporalGridScope grid_scope(ctx, s);
        // the keyframe's refined depths, when they are in use and a frame has been fused (at the prior lambda is 1)
        const double *d_lam = ctx->use_depth && !ctx->kf_depth_fresh ? ctx->kf_lambda : nullptr;
        rc = align_run(ctx, s, ctx->kf_L, ctx->kf_R, n_kf, s.im[0].edges, n0, s.im[1].edges, n1, s.cur_w, s.cur_h, cal, params, R0, t0, d_lam,
                       &r, assoc_left, assoc_right);
    }
    if (rc)
        return rc;
    align_publish(r, n_kf, out);
    return EBVO_OK;
}

// ---- inverse-depth filter of the keyframe mates (depth_kernels.hip) -----------------------------------------------------
extern "C" void ebvo_depth_default_params(ebvo_depth_params *p)
{
    if (!p)
        return;
    p->sigma_disp_px = 0.25;
    p->sigma_normal_px = 0.5;
    p->huber_px = 1.0;
    p->gate_px = 3.0;
    p->iterations = 3;
    p->cameras = 2;
    p->lambda_min = 0.25;
    p->lambda_max = 4.0;
    p->info_max = 1e6;
    p->img_margin = 10.0;
    p->block_threads = 0;
    p->reserved = 0;
}

static bool depth_args_ok(const ebvo_stereo_calib *cal, const ebvo_depth_params *dp, const double *R, const double *t,
                          const ebvo_depth_refined *out, int img_w, int img_h)
{
    if (!cal || !dp || !R || !t || !out || img_w < 1 || img_h < 1)
        return false;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R[i]))
            return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(t[i]))
            return false;
    const int bt = dp->block_threads;
    // every comparison is false for a NaN
    return std::isfinite(dp->sigma_disp_px) && dp->sigma_disp_px > 0 && std::isfinite(dp->sigma_normal_px) && dp->sigma_normal_px > 0 &&
           dp->huber_px > 0 && dp->gate_px > 0 && dp->iterations >= 0 && dp->iterations <= 16 && std::isfinite(dp->lambda_max) &&
           dp->lambda_min > 0 && dp->lambda_min <= dp->lambda_max && dp->info_max > 0 && dp->img_margin >= 0 &&
           (dp->cameras == 1 || dp->cameras == 2) && (bt == 0 || bt == 256 || bt == 512 || bt == 1024) && dp->reserved == 0;
}

static void depth_publish(const DepthRecord &r, int n_kf, ebvo_depth_refined *out)
{
    memset(out, 0, sizeof *out);
    out->n_kf = n_kf;
    out->n_dead = r.n_dead;
    out->n_updated = r.n_updated;
    out->n_restored = r.n_restored;
    for (int c = 0; c < 2; ++c)
    {
        out->n_terms[c] = r.n_terms[c];
        out->n_gated[c] = r.n_gated[c];
    }
    out->rms_before = r.rms_before;
    out->rms_after = r.rms_after;
}

extern "C" int ebvo_depth_refine_edges(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf,
                                       const ebvo_edge *cf_edges_left, int n0, const ebvo_edge *cf_edges_right, int n1,
                                       const int32_t *assoc_left, const int32_t *assoc_right, int img_w, int img_h,
                                       const ebvo_stereo_calib *cal, const ebvo_depth_params *params, const double R[9], const double t[3],
                                       const double *lambda_in, const double *info_in, const int32_t *n_obs_in, double *lambda,
                                       double *info, int32_t *n_obs, uint8_t *flags, ebvo_depth_refined *out)
{
    if (!ctx || !depth_args_ok(cal, params, R, t, out, img_w, img_h) || n_kf < 0 || n0 < 0 ||
        (n_kf > 0 && (!kf_left || !kf_right || !lambda || !info || !n_obs || !flags)) || (n0 > 0 && !cf_edges_left))
        return EBVO_ERR_ARG;
    const int have_in = (lambda_in ? 1 : 0) + (info_in ? 1 : 0) + (n_obs_in ? 1 : 0);
    if (have_in != 0 && have_in != 3)
        return EBVO_ERR_ARG;
    if (params->cameras == 1)
        n1 = 0;
    else if (n1 < 0 || (n1 > 0 && !cf_edges_right))
        return EBVO_ERR_ARG;
    DepthRecord r;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    if (n_kf == 0)
    {
        memset(out, 0, sizeof *out);
        return EBVO_OK;
    }
    const size_t nz = (size_t)n_kf, eb = sizeof(ebvo_edge);
    Carve L;
    const size_t o_kfL = L.take(eb * nz), o_kfR = L.take(eb * nz), o_E0 = L.take(eb * (size_t)n0), o_E1 = L.take(eb * (size_t)n1),
                 o_a0 = L.take(4 * nz), o_a1 = L.take(4 * nz), o_lam = L.take(8 * nz), o_info = L.take(8 * nz), o_nobs = L.take(4 * nz),
                 o_fl = L.take(nz);
    if (hc.stage(L))
        return hc.rc;
    ebvo_edge *kfL = hc.at<ebvo_edge>(o_kfL), *kfR = hc.at<ebvo_edge>(o_kfR), *E0 = hc.at<ebvo_edge>(o_E0), *E1 = hc.at<ebvo_edge>(o_E1);
    int32_t *a0 = assoc_left ? hc.at<int32_t>(o_a0) : nullptr, *a1 = params->cameras > 1 && assoc_right ? hc.at<int32_t>(o_a1) : nullptr;
    int32_t *d_nobs = hc.at<int32_t>(o_nobs);
    double *d_lam = hc.at<double>(o_lam), *d_info = hc.at<double>(o_info);
    uint8_t *d_fl = hc.at<uint8_t>(o_fl);
    if (hc.up(kfL, kf_left, eb * nz) || hc.up(kfR, kf_right, eb * nz) || hc.up(E0, cf_edges_left, eb * (size_t)n0) ||
        hc.up(E1, cf_edges_right, eb * (size_t)n1) || hc.up(a0, assoc_left, 4 * nz) || hc.up(a1, assoc_right, a1 ? 4 * nz : 0) ||
        hc.up(d_lam, lambda_in, 8 * nz) || hc.up(d_info, info_in, 8 * nz) || hc.up(d_nobs, n_obs_in, 4 * nz))
        return hc.rc;
    {
        const TemporalGridScope grid_scope(ctx, hc.slot());
        if (int rc = depth_run(ctx, hc.slot(), kfL, kfR, n_kf, E0, n0, E1, n1, a0, a1, img_w, img_h, cal, params, R, t,
                               have_in ? d_lam : nullptr, have_in ? d_info : nullptr, have_in ? d_nobs : nullptr, d_lam, d_info, d_nobs, d_fl,
                               &r))
            return rc;
    }
    hc.down(lambda, d_lam, 8 * nz);
    hc.down(info, d_info, 8 * nz);
    hc.down(n_obs, d_nobs, 4 * nz);
    hc.down(flags, d_fl, nz);
    if (hc.finish())
        return hc.rc;
    depth_publish(r, n_kf, out);
    return EBVO_OK;
}

// the keyframe's state arrays hold kf_n values
static int depth_state_ensure(ebvo_ctx *ctx)
{
    const size_t n = (size_t)ctx->kf_n;
    if (n <= ctx->kf_depth_cap && ctx->kf_lambda)
        return EBVO_OK;
    EBVO_HIP(ctx, hipDeviceSynchronize());
    for (void *p : {(void *)ctx->kf_lambda, (void *)ctx->kf_info, (void *)ctx->kf_nobs, (void *)ctx->kf_dflags})
        (void)hipFree(p);
    ctx->kf_lambda = ctx->kf_info = nullptr;
    ctx->kf_nobs = nullptr;
    ctx->kf_dflags = nullptr;
    ctx->kf_depth_cap = 0;
    ctx->kf_depth_fresh = true;
    const size_t cap = n + n / 4 + 64;
    if (hipMalloc(&ctx->kf_lambda, 8 * cap) != hipSuccess || hipMalloc(&ctx->kf_info, 8 * cap) != hipSuccess ||
        hipMalloc(&ctx->kf_nobs, 4 * cap) != hipSuccess || hipMalloc(&ctx->kf_dflags, cap) != hipSuccess)
    {
        (void)hipGetLastError();
        ctx->last_error = "hipMalloc failed (keyframe depth state)";
        return EBVO_ERR_NOMEM;
    }
    ctx->kf_depth_cap = cap;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_refine_depth(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_align_params *align_params,
                                          const ebvo_depth_params *depth_params, const double R[9], const double t[3],
                                          ebvo_depth_refined *out)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    const int w = s.have_run ? s.cur_w : 1, h = s.have_run ? s.cur_h : 1;
    ebvo_aligned_pose unused;
    if (!depth_args_ok(cal, depth_params, R, t, out, w, h) || !align_args_ok(cal, align_params, R, t, &unused, w, h))
        return EBVO_ERR_ARG;
    if (int rc = align_slot_state(ctx, s))
        return rc;
    const int n_kf = ctx->kf_n, n0 = s.im[0].n_kept, n1 = depth_params->cameras > 1 ? s.im[1].n_kept : 0;
    if (n_kf == 0)
    {
        memset(out, 0, sizeof *out);
        return EBVO_OK;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = depth_state_ensure(ctx))
        return rc;
    ebvo_align_params ap = *align_params;
    ap.cameras = depth_params->cameras;
    const bool fresh = ctx->kf_depth_fresh;
    DepthRecord r;
    int rc;
    {
        const TemporalGridScope grid_scope(ctx, s);
        const int32_t *idx0 = nullptr, *idx1 = nullptr;
        rc = EBVO_OK;
        if (n0 + (int64_t)n1 > 0) // without an edge nothing can be associated: every live mate is restored
            rc = align_associate_once(ctx, s, ctx->kf_L, ctx->kf_R, n_kf, s.im[0].edges, n0, s.im[1].edges, n1, s.cur_w, s.cur_h, cal, &ap, R, t,
                                      fresh ? nullptr : ctx->kf_lambda, &idx0, &idx1);
        if (!rc)
            rc = depth_run(ctx, s, ctx->kf_L, ctx->kf_R, n_kf, s.im[0].edges, n0, s.im[1].edges, n1, idx0, idx1, s.cur_w, s.cur_h, cal,
                           depth_params, R, t, fresh ? nullptr : ctx->kf_lambda, fresh ? nullptr : ctx->kf_info,
                           fresh ? nullptr : ctx->kf_nobs, ctx->kf_lambda, ctx->kf_info, ctx->kf_nobs, ctx->kf_dflags, &r);
    }
    const hipError_t e = hipStreamSynchronize(s.stream);
    if (rc)
        return rc;
    EBVO_HIP(ctx, e);
    ctx->kf_depth_fresh = false;
    depth_publish(r, n_kf, out);
    return EBVO_OK;
}

extern "C" int ebvo_temporal_depth_fetch(ebvo_ctx *ctx, double *lambda, double *info, int32_t *n_obs, uint8_t *flags)
{
    if (!ctx)
        return EBVO_ERR_ARG;
    if (ctx->kf_n < 0)
    {
        ctx->last_error = "no keyframe (ebvo_temporal_set_keyframe first)";
        return EBVO_ERR_STATE;
    }
    const size_t n = (size_t)ctx->kf_n;
    if (ctx->kf_depth_fresh || n == 0)
    {
        for (size_t i = 0; i < n; ++i)
        {
            if (lambda)
                lambda[i] = 1.0;
            if (info)
                info[i] = 0.0;
            if (n_obs)
                n_obs[i] = 0;
            if (flags)
                flags[i] = 0;
        }
        return EBVO_OK;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    // every call that writes the state waits for its stream before it returns
    if (lambda)
        EBVO_HIP(ctx, hipMemcpy(lambda, ctx->kf_lambda, 8 * n, hipMemcpyDeviceToHost));
    if (info)
        EBVO_HIP(ctx, hipMemcpy(info, ctx->kf_info, 8 * n, hipMemcpyDeviceToHost));
    if (n_obs)
        EBVO_HIP(ctx, hipMemcpy(n_obs, ctx->kf_nobs, 4 * n, hipMemcpyDeviceToHost));
    if (flags)
        EBVO_HIP(ctx, hipMemcpy(flags, ctx->kf_dflags, n, hipMemcpyDeviceToHost));
    return EBVO_OK;
}

extern "C" int ebvo_temporal_depth_reset(ebvo_ctx *ctx)
{
    if (!ctx)
        return EBVO_ERR_ARG;
    if (ctx->kf_n < 0)
    {
        ctx->last_error = "no keyframe (ebvo_temporal_set_keyframe first)";
        return EBVO_ERR_STATE;
    }
    ctx->kf_depth_fresh = true;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_use_depth(ebvo_ctx *ctx, int on)
{
    if (!ctx)
        return EBVO_ERR_ARG;
    ctx->use_depth = on != 0;
    return EBVO_OK;
}

// ---- handover of the refined depths to the next keyframe on promotion (carry_kernels.hip) --------------------------------
extern "C" void ebvo_depth_carry_default_params(ebvo_depth_carry_params *p)
{
    if (!p)
        return;
    p->sigma_disp_px = 0.25;
    p->radius = 1.5;
    p->cell_size = 4;
    p->min_obs = 1;
    p->orient_thr_deg = 10.0;
    p->carry = 0.5;
    p->gate_sigmas = 3.0;
    p->lambda_min = 0.25;
    p->lambda_max = 4.0;
    p->info_max = 1e6;
    p->img_margin = 10.0;
    p->reserved = 0;
    p->pad = 0;
}

static bool carry_args_ok(const ebvo_stereo_calib *cal, const ebvo_depth_carry_params *cp, const double *R, const double *t,
                          const ebvo_depth_carried *out, int img_w, int img_h)
{
    if (!cal || !cp || !R || !t || !out || img_w < 1 || img_h < 1)
        return false;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R[i]))
            return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(t[i]))
            return false;
    // every comparison is false for a NaN
    if (!(std::isfinite(cp->sigma_disp_px) && cp->sigma_disp_px > 0 && std::isfinite(cp->radius) && cp->radius > 0 && cp->cell_size >= 1 &&
          cp->min_obs >= 0 && cp->orient_thr_deg >= 0 && cp->carry > 0 && cp->carry <= 1 && cp->gate_sigmas > 0 &&
          std::isfinite(cp->lambda_max) && cp->lambda_min > 0 && cp->lambda_min <= cp->lambda_max && cp->info_max > 0 &&
          cp->img_margin >= 0 && cp->reserved == 0 && cp->pad == 0))
        return false;
    if (!(ceil(cp->radius / cp->cell_size) <= 8.0))
        return false;
    const int64_t gw = ((int64_t)img_w + cp->cell_size - 1) / cp->cell_size, gh = ((int64_t)img_h + cp->cell_size - 1) / cp->cell_size;
    return gw * gh <= (1 << 26);
}

static void carry_publish(const int32_t *counts, int n_old, int n_new, ebvo_depth_carried *out)
{
    out->n_old = n_old;
    out->n_sources = counts[0];
    out->n_live = counts[1];
    out->n_new = n_new;
    out->n_dead = counts[2];
    out->n_assoc = counts[3];
    out->n_carried = counts[4];
    out->n_gated = counts[5];
}

extern "C" int ebvo_depth_carry(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_old, const double *lambda_in,
                                const double *info_in, const int32_t *n_obs_in, const ebvo_edge *new_left, const ebvo_edge *new_right,
                                int n_new, int img_w, int img_h, const ebvo_stereo_calib *cal, const ebvo_depth_carry_params *params,
                                const double R[9], const double t[3], double *lambda, double *info, int32_t *n_obs, uint8_t *flags,
                                int32_t *src_index, ebvo_depth_carried *out)
{
    if (!ctx || !carry_args_ok(cal, params, R, t, out, img_w, img_h) || n_old < 0 || n_new < 0 || (n_old > 0 && (!kf_left || !kf_right)) ||
        (n_new > 0 && (!new_left || !new_right || !lambda || !info || !n_obs || !flags || !src_index)))
        return EBVO_ERR_ARG;
    const int have_in = (lambda_in ? 1 : 0) + (info_in ? 1 : 0) + (n_obs_in ? 1 : 0);
    if (have_in != 0 && have_in != 3)
        return EBVO_ERR_ARG;
    int32_t counts[CARRY_COUNTS] = {0, 0, 0, 0, 0, 0};
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    if (n_new == 0)
    {
        carry_publish(counts, n_old, n_new, out);
        return EBVO_OK;
    }
    const bool assoc = have_in && n_old > 0;
    const size_t no = assoc ? (size_t)n_old : 0, nn = (size_t)n_new, eb = sizeof(ebvo_edge);
    // old mates and their state, new mates, the outgoing state
    Carve L;
    const size_t o_oL = L.take(eb * no), o_oR = L.take(eb * no), o_li = L.take(8 * no), o_ii = L.take(8 * no), o_ni = L.take(4 * no),
                 o_nL = L.take(eb * nn), o_nR = L.take(eb * nn), o_lam = L.take(8 * nn), o_info = L.take(8 * nn), o_nobs = L.take(4 * nn),
                 o_src = L.take(4 * nn), o_fl = L.take(nn);
    if (hc.stage(L))
        return hc.rc;
    ebvo_edge *oL = hc.at<ebvo_edge>(o_oL), *oR = hc.at<ebvo_edge>(o_oR), *nL = hc.at<ebvo_edge>(o_nL), *nR = hc.at<ebvo_edge>(o_nR);
    double *d_li = hc.at<double>(o_li), *d_ii = hc.at<double>(o_ii), *d_lam = hc.at<double>(o_lam), *d_info = hc.at<double>(o_info);
    int32_t *d_ni = hc.at<int32_t>(o_ni), *d_nobs = hc.at<int32_t>(o_nobs), *d_src = hc.at<int32_t>(o_src);
    uint8_t *d_fl = hc.at<uint8_t>(o_fl);
    if (hc.up(oL, kf_left, eb * no) || hc.up(oR, kf_right, eb * no) || hc.up(d_li, lambda_in, 8 * no) || hc.up(d_ii, info_in, 8 * no) ||
        hc.up(d_ni, n_obs_in, 4 * no) || hc.up(nL, new_left, eb * nn) || hc.up(nR, new_right, eb * nn))
        return hc.rc;
    {
        const TemporalGridScope grid_scope(ctx, hc.slot());
        if (int rc = carry_run(ctx, hc.slot(), oL, oR, n_old, assoc ? d_li : nullptr, assoc ? d_ii : nullptr, assoc ? d_ni : nullptr, nL, nR,
                               n_new, img_w, img_h, cal, params, R, t, d_lam, d_info, d_nobs, d_fl, d_src, counts))
            return rc;
    }
    hc.down(lambda, d_lam, 8 * nn);
    hc.down(info, d_info, 8 * nn);
    hc.down(n_obs, d_nobs, 4 * nn);
    hc.down(flags, d_fl, nn);
    hc.down(src_index, d_src, 4 * nn);
    if (hc.finish())
        return hc.rc;
    carry_publish(counts, n_old, n_new, out);
    return EBVO_OK;
}

// (R, t) after (Rk, tk): Ro = R Rk, every entry (R_i0 Rk_0j + R_i1 Rk_1j) + R_i2 Rk_2j, and to = mv3(R, tk) + t; one rounding
// per operation (-ffp-contract=off holds for the host code of this file too)
static void seq_compose(const double *R, const double *t, const double *Rk, const double *tk, double *Ro, double *to)
{
    for (int i = 0; i < 3; ++i)
    {
        for (int j = 0; j < 3; ++j)
            Ro[3 * i + j] = (R[3 * i] * Rk[j] + R[3 * i + 1] * Rk[3 + j]) + R[3 * i + 2] * Rk[6 + j];
        to[i] = ((R[3 * i] * tk[0] + R[3 * i + 1] * tk[1]) + R[3 * i + 2] * tk[2]) + t[i];
    }
}

// the second set of state arrays holds n values (the set the next promotion writes)
static int carry_alt_ensure(ebvo_ctx *ctx, size_t n)
{
    if (n <= ctx->kf_depth_alt_cap && n <= ctx->kf_src_alt_cap && ctx->kf_lambda_alt && ctx->kf_src_alt)
        return EBVO_OK;
    EBVO_HIP(ctx, hipDeviceSynchronize());
    for (void *p : {(void *)ctx->kf_lambda_alt, (void *)ctx->kf_info_alt, (void *)ctx->kf_nobs_alt, (void *)ctx->kf_dflags_alt,
                    (void *)ctx->kf_src_alt})
        (void)hipFree(p);
    ctx->kf_lambda_alt = ctx->kf_info_alt = nullptr;
    ctx->kf_nobs_alt = ctx->kf_src_alt = nullptr;
    ctx->kf_dflags_alt = nullptr;
    ctx->kf_depth_alt_cap = ctx->kf_src_alt_cap = 0;
    const size_t cap = n + n / 4 + 64;
    if (hipMalloc(&ctx->kf_lambda_alt, 8 * cap) != hipSuccess || hipMalloc(&ctx->kf_info_alt, 8 * cap) != hipSuccess ||
        hipMalloc(&ctx->kf_nobs_alt, 4 * cap) != hipSuccess || hipMalloc(&ctx->kf_dflags_alt, cap) != hipSuccess ||
        hipMalloc(&ctx->kf_src_alt, 4 * cap) != hipSuccess)
    {
        (void)hipGetLastError();
        ctx->last_error = "hipMalloc failed (carried depth state)";
        return EBVO_ERR_NOMEM;
    }
    ctx->kf_depth_alt_cap = ctx->kf_src_alt_cap = cap;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_promote_keyframe(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_depth_carry_params *params,
                                              const double R[9], const double t[3], ebvo_depth_carried *out)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    // the frame's size enters the accepted ranges through the grid; a slot without a pair has none yet
    if (!carry_args_ok(cal, params, R, t, out, s.have_run ? s.cur_w : 1, s.have_run ? s.cur_h : 1))
        return EBVO_ERR_ARG;
    if (ctx->kf_n < 0)
    {
        ctx->last_error = "no keyframe to promote from (ebvo_temporal_set_keyframe first)";
        return EBVO_ERR_STATE;
    }
    if (int rc = keyframe_slot_state(ctx, s))
        return rc;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = drain_fetch(ctx, s))
        return rc;
    const int n_old = ctx->kf_n, n_new = s.n_final;
    // an old keyframe at the prior has nothing to carry
    const bool carry = !ctx->kf_depth_fresh && n_old > 0 && n_new > 0;
    int32_t counts[CARRY_COUNTS] = {0, 0, 0, 0, 0, 0};
    if (carry)
    {
        if (int rc = carry_alt_ensure(ctx, (size_t)n_new))
            return rc;
        const ebvo_edge *fl, *fr;
        final_mates(s, &fl, &fr);
        // behind these launches, on the same stream, the installation overwrites the store they read
        const TemporalGridScope grid_scope(ctx, s);
        const int rc = carry_run(ctx, s, ctx->kf_L, ctx->kf_R, n_old, ctx->kf_lambda, ctx->kf_info, ctx->kf_nobs, fl, fr, n_new, s.cur_w, s.cur_h,
                                 cal, params, R, t, ctx->kf_lambda_alt, ctx->kf_info_alt, ctx->kf_nobs_alt, ctx->kf_dflags_alt, ctx->kf_src_alt,
                                 counts);
        if (rc)
        {
            (void)hipStreamSynchronize(s.stream);
            return rc;
        }
    }
    if (int rc = keyframe_install(ctx, s))
    {
        (void)hipStreamSynchronize(s.stream); // the counters' copy writes this frame's stack
        return rc;
    }
    if (carry)
    {
        std::swap(ctx->kf_lambda, ctx->kf_lambda_alt);
        std::swap(ctx->kf_info, ctx->kf_info_alt);
        std::swap(ctx->kf_nobs, ctx->kf_nobs_alt);
        std::swap(ctx->kf_dflags, ctx->kf_dflags_alt);
        std::swap(ctx->kf_depth_cap, ctx->kf_depth_alt_cap);
        std::swap(ctx->kf_src, ctx->kf_src_alt);
        std::swap(ctx->kf_src_cap, ctx->kf_src_alt_cap);
        ctx->kf_depth_fresh = false;
    }
    ctx->kf_promoted = true;
    ctx->kf_src_none = !carry;
    carry_publish(counts, n_old, n_new, out);
    // the new keyframe's pose in the sequence frame: Rk <- R Rk, tk <- R tk + t
    double Rk[9], tk[3];
    seq_compose(R, t, ctx->kf_Rk, ctx->kf_tk, Rk, tk);
    memcpy(ctx->kf_Rk, Rk, sizeof Rk);
    memcpy(ctx->kf_tk, tk, sizeof tk);
    return EBVO_OK;
}

extern "C" int ebvo_temporal_depth_source(ebvo_ctx *ctx, int32_t *src_index)
{
    if (!ctx)
        return EBVO_ERR_ARG;
    if (ctx->kf_n < 0 || !ctx->kf_promoted)
    {
        ctx->last_error = "the keyframe was not installed by ebvo_temporal_promote_keyframe";
        return EBVO_ERR_STATE;
    }
    const size_t n = (size_t)ctx->kf_n;
    if (!src_index || n == 0)
        return EBVO_OK;
    if (ctx->kf_src_none)
    {
        for (size_t i = 0; i < n; ++i)
            src_index[i] = -1;
        return EBVO_OK;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    EBVO_HIP(ctx, hipMemcpy(src_index, ctx->kf_src, 4 * n, hipMemcpyDeviceToHost));
    return EBVO_OK;
}

// ---- keyframe coverage, the switch policy and the frame step (cover_kernels.hip) ------------------------------------------
extern "C" void ebvo_cover_default_params(ebvo_cover_params *p)
{
    if (!p)
        return;
    p->radius = 4.0;
    p->orient_thr_deg = 10.0;
    p->img_margin = 10.0;
    p->inlier_px = 1.0;
    p->bin_px = 1.0;
    p->cell_size = 4;
    p->cover_cell = 32;
    p->min_cell_edges = 4;
    p->min_cell_explained = 2;
    p->reserved = 0;
    p->pad = 0;
}

static bool cover_args_ok(const ebvo_stereo_calib *cal, const ebvo_cover_params *cp, const double *R, const double *t,
                          const ebvo_keyframe_cover *out, int img_w, int img_h)
{
    if (!cal || !cp || !R || !t || !out || img_w < 1 || img_h < 1)
        return false;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R[i]))
            return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(t[i]))
            return false;
    // every comparison is false for a NaN
    if (!(std::isfinite(cp->radius) && cp->radius > 0 && cp->cell_size >= 1 && cp->orient_thr_deg >= 0 && cp->img_margin >= 0 &&
          cp->inlier_px >= 0 && std::isfinite(cp->bin_px) && cp->bin_px > 0 && cp->cover_cell >= 1 && cp->min_cell_edges >= 1 &&
          cp->min_cell_explained >= 1 && cp->reserved == 0 && cp->pad == 0))
        return false;
    if (!(ceil(cp->radius / cp->cell_size) <= 8.0))
        return false;
    const int64_t gw = ((int64_t)img_w + cp->cell_size - 1) / cp->cell_size, gh = ((int64_t)img_h + cp->cell_size - 1) / cp->cell_size;
    const int64_t cw = ((int64_t)img_w + cp->cover_cell - 1) / cp->cover_cell, ch = ((int64_t)img_h + cp->cover_cell - 1) / cp->cover_cell;
    return gw * gh <= (1 << 26) && cw * ch <= (1 << 26);
}

// nothing to launch: the record and every output that was asked for
static void cover_nothing(const ebvo_cover_params *cp, int n_kf, int n0, int img_w, int img_h, ebvo_keyframe_cover *out, uint8_t *flags,
                          int32_t *assoc, double *disp, uint8_t *explained, int32_t *cell_edges, int32_t *cell_explained)
{
    memset(out, 0, sizeof *out);
    out->n_kf = n_kf;
    out->n_edges = n0;
    out->cw = (int32_t)(((int64_t)img_w + cp->cover_cell - 1) / cp->cover_cell);
    out->ch = (int32_t)(((int64_t)img_h + cp->cover_cell - 1) / cp->cover_cell);
    out->disp_median_bin = -1;
    for (int i = 0; i < n_kf; ++i)
    {
        if (flags)
            flags[i] = 0;
        if (assoc)
            assoc[i] = -1;
        if (disp)
            disp[i] = NAN;
    }
    if (explained && n0 > 0)
        memset(explained, 0, (size_t)n0);
    const size_t nc = (size_t)out->cw * (size_t)out->ch;
    if (cell_edges)
        memset(cell_edges, 0, sizeof(int32_t) * nc);
    if (cell_explained)
        memset(cell_explained, 0, sizeof(int32_t) * nc);
}

extern "C" int ebvo_keyframe_cover_edges(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, const double *lambda, int n_kf,
                                         const ebvo_edge *cf_edges_left, int n0, int img_w, int img_h, const ebvo_stereo_calib *cal,
                                         const ebvo_cover_params *params, const double R[9], const double t[3], ebvo_keyframe_cover *out,
                                         uint8_t *flags, int32_t *assoc, double *disp, uint8_t *explained, int32_t *cell_edges,
                                         int32_t *cell_explained)
{
    if (!ctx || !cover_args_ok(cal, params, R, t, out, img_w, img_h) || n_kf < 0 || n0 < 0 || (n_kf > 0 && (!kf_left || !kf_right)) ||
        (n0 > 0 && !cf_edges_left))
        return EBVO_ERR_ARG;
    ebvo_keyframe_cover rec;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    if (n_kf == 0 || n0 == 0)
    {
        cover_nothing(params, n_kf, n0, img_w, img_h, out, flags, assoc, disp, explained, cell_edges, cell_explained);
        return EBVO_OK;
    }
    const size_t nz = (size_t)n_kf, eb = sizeof(ebvo_edge);
    Carve L;
    const size_t o_kfL = L.take(eb * nz), o_kfR = L.take(eb * nz), o_E0 = L.take(eb * (size_t)n0), o_lam = L.take(8 * nz);
    if (hc.stage(L))
        return hc.rc;
    ebvo_edge *kfL = hc.at<ebvo_edge>(o_kfL), *kfR = hc.at<ebvo_edge>(o_kfR), *E0 = hc.at<ebvo_edge>(o_E0);
    double *d_lam = lambda ? hc.at<double>(o_lam) : nullptr;
    if (hc.up(kfL, kf_left, eb * nz) || hc.up(kfR, kf_right, eb * nz) || hc.up(E0, cf_edges_left, eb * (size_t)n0) ||
        hc.up(d_lam, lambda, 8 * nz))
        return hc.rc;
    {
        const TemporalGridScope grid_scope(ctx, hc.slot());
        if (int rc = cover_run(ctx, hc.slot(), kfL, kfR, n_kf, d_lam, E0, n0, img_w, img_h, cal, params, R, t, &rec, flags, assoc, disp,
                               explained, cell_edges, cell_explained))
            return rc;
    }
    if (hc.finish())
        return hc.rc;
    *out = rec;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_keyframe_cover(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_cover_params *params,
                                            const double R[9], const double t[3], ebvo_keyframe_cover *out, uint8_t *flags, int32_t *assoc,
                                            double *disp, uint8_t *explained, int32_t *cell_edges, int32_t *cell_explained)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    // the frame's size enters the accepted ranges through the grids; a slot without a pair has none yet
    if (!cover_args_ok(cal, params, R, t, out, s.have_run ? s.cur_w : 1, s.have_run ? s.cur_h : 1))
        return EBVO_ERR_ARG;
    if (int rc = align_slot_state(ctx, s))
        return rc;
    const int n_kf = ctx->kf_n, n0 = s.im[0].n_kept;
    if (n_kf == 0 || n0 == 0)
    {
        cover_nothing(params, n_kf, n0, s.cur_w, s.cur_h, out, flags, assoc, disp, explained, cell_edges, cell_explained);
        return EBVO_OK;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    ebvo_keyframe_cover rec;
    int rc;
    {
        const TemporalGridScope grid_scope(ctx, s);
        // the keyframe's refined depths, when they are in use and a frame has been fused (at the prior lambda is 1)
        const double *d_lam = ctx->use_depth && !ctx->kf_depth_fresh ? ctx->kf_lambda : nullptr;
        rc = cover_run(ctx, s, ctx->kf_L, ctx->kf_R, n_kf, d_lam, s.im[0].edges, n0, s.cur_w, s.cur_h, cal, params, R, t, &rec, flags, assoc, disp,
                       explained, cell_edges, cell_explained);
    }
    const hipError_t e = hipStreamSynchronize(s.stream);
    if (rc)
        return rc;
    EBVO_HIP(ctx, e);
    *out = rec;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_cover_size(ebvo_ctx *ctx, int slot, const ebvo_cover_params *params, int32_t *n_kf, int32_t *n0, int32_t *cw,
                                        int32_t *ch)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp) || !params || params->cover_cell < 1 || !n_kf || !n0 || !cw || !ch)
        return EBVO_ERR_ARG;
    if (int rc = align_slot_state(ctx, *sp))
        return rc;
    *n_kf = ctx->kf_n;
    *n0 = sp->im[0].n_kept;
    *cw = (int32_t)(((int64_t)sp->cur_w + params->cover_cell - 1) / params->cover_cell);
    *ch = (int32_t)(((int64_t)sp->cur_h + params->cover_cell - 1) / params->cover_cell);
    return EBVO_OK;
}

extern "C" void ebvo_keyframe_policy_default(ebvo_keyframe_policy *p)
{
    if (!p)
        return;
    p->min_assoc = 50;
    p->max_disp_bins = 30;
    p->min_in_frame_share = 0.7;
    p->min_assoc_share = 0.5;
    p->min_cell_cover = 0.6;
}

extern "C" int ebvo_keyframe_decide(const ebvo_keyframe_cover *c, const ebvo_keyframe_policy *p, uint32_t *reasons)
{
    if (!c || !p)
        return EBVO_ERR_ARG;
    uint32_t r = 0;
    if (c->n_assoc < p->min_assoc)
        r |= EBVO_KF_LOST;
    if ((double)c->n_in_frame < p->min_in_frame_share * (double)(c->n_kf - c->n_dead))
        r |= EBVO_KF_LOW_OVERLAP;
    if ((double)c->n_assoc < p->min_assoc_share * (double)c->n_in_frame)
        r |= EBVO_KF_LOW_ASSOC;
    if ((double)c->n_cells_covered < p->min_cell_cover * (double)c->n_cells_cur)
        r |= EBVO_KF_NEW_CONTENT;
    if (c->disp_median_bin >= p->max_disp_bins)
        r |= EBVO_KF_PARALLAX;
    if (reasons)
        *reasons = r;
    return (r & EBVO_KF_LOST) ? 2 : r ? 1 : 0;
}

extern "C" int ebvo_temporal_keyframe_pose(ebvo_ctx *ctx, double R[9], double t[3])
{
    if (!ctx)
        return EBVO_ERR_ARG;
    if (ctx->kf_n < 0)
    {
        ctx->last_error = "no keyframe (ebvo_temporal_set_keyframe first)";
        return EBVO_ERR_STATE;
    }
    if (R)
        memcpy(R, ctx->kf_Rk, sizeof ctx->kf_Rk);
    if (t)
        memcpy(t, ctx->kf_tk, sizeof ctx->kf_tk);
    return EBVO_OK;
}

extern "C" void ebvo_track_default_params(ebvo_track_params *p)
{
    if (!p)
        return;
    memset(p, 0, sizeof *p);
    ebvo_align_default_params(&p->align);
    ebvo_depth_default_params(&p->depth);
    ebvo_cover_default_params(&p->cover);
    ebvo_depth_carry_default_params(&p->carry);
    ebvo_finalize_default_params(&p->finalize);
    ebvo_keyframe_policy_default(&p->policy);
    p->refine_depth = 1;
    p->reserved = 0;
}

extern "C" int ebvo_temporal_track_frame(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_track_params *params,
                                         const double R0[9], const double t0[3], ebvo_tracked_frame *out)
{
    if (!ctx || !params || !out || (params->refine_depth != 0 && params->refine_depth != 1) || params->reserved != 0)
        return EBVO_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->cover.disp_median_bin = -1;
    out->decision = 2;
    int rc;
    auto failed = [&](int stage, int status) {
        out->failed_stage = stage;
        return status;
    };
    // (a) the pose
    if ((rc = ebvo_temporal_align_pose(ctx, slot, cal, &params->align, R0, t0, &out->pose, nullptr, nullptr)))
        return failed(EBVO_TRACK_STAGE_ALIGN, rc);
    const double *R = out->pose.R, *t = out->pose.t;
    seq_compose(R, t, ctx->kf_Rk, ctx->kf_tk, out->R_seq, out->t_seq);
    if (out->pose.status != 0)
        return EBVO_OK; // tracking lost: tracked 0, decision 2
    out->tracked = 1;
    // (b) the keyframe's depths
    if (params->refine_depth && (rc = ebvo_temporal_refine_depth(ctx, slot, cal, &params->align, &params->depth, R, t, &out->depth)))
        return failed(EBVO_TRACK_STAGE_DEPTH, rc);
    // (c) the measurement, (d) the decision
    if ((rc = ebvo_temporal_keyframe_cover(ctx, slot, cal, &params->cover, R, t, &out->cover, nullptr, nullptr, nullptr, nullptr, nullptr,
                                           nullptr)))
        return failed(EBVO_TRACK_STAGE_COVER, rc);
    out->decision = ebvo_keyframe_decide(&out->cover, &params->policy, &out->reasons);
    if (out->decision != 1)
        return EBVO_OK;
    // (e) the switch
    if ((rc = ebvo_stereo_finalize(ctx, slot, &params->finalize, cal, &out->finalized)))
        return failed(EBVO_TRACK_STAGE_FINALIZE, rc);
    if ((rc = ebvo_temporal_promote_keyframe(ctx, slot, cal, &params->carry, R, t, &out->carried)))
        return failed(EBVO_TRACK_STAGE_PROMOTE, rc);
    out->switched = 1;
    return EBVO_OK;
}

// the slot's page-locked result arena holds at least `bytes` (a re-allocation waits for copies still heading into the old one).
// It exists even for zero bytes: a selected array of a pair without edges or pairs is an empty array, not a NULL pointer
// (NULL in a view means "not selected").
static int ensure_arena(ebvo_ctx *ctx, Slot &s, size_t bytes)
{
    if (bytes <= s.h_arena_bytes && s.h_arena)
        return EBVO_OK;
    if (s.fetch_pending)
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_rebind));
    if (s.h_arena)
        (void)hipHostFree(s.h_arena);
    s.h_arena = nullptr;
    s.h_arena_bytes = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&s.h_arena, want) != hipSuccess)
    {
        (void)hipGetLastError();
        ctx->last_error = "hipHostMalloc failed (page-locked result staging)";
        return EBVO_ERR_NOMEM;
    }
    s.h_arena_bytes = want;
    return EBVO_OK;
}

// ---- results through page-locked memory, no staging copy on the host ------------------------------------------------
extern "C" int ebvo_stereo_fetch_begin(ebvo_ctx *ctx, int slot, int what)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp) || what <= 0 || (what & ~EBVO_FETCH_ALL))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_run || s.in_flight)
        return EBVO_ERR_STATE;
    if ((what & EBVO_FETCH_SIMS) && !s.have_sims)
    {
        ctx->last_error = "the pair was submitted with EBVO_PAIR_NO_SIMS: the four scores were not stored";
        return EBVO_ERR_STATE;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nL = (size_t)s.result.n_left, nR = (size_t)s.result.n_right, np = (size_t)s.result.n_pairs;
    const size_t sizes[7] = {(what & EBVO_FETCH_EDGES) ? sizeof(ebvo_edge) * nL : 0,
                             (what & EBVO_FETCH_EDGES) ? sizeof(ebvo_edge) * nR : 0,
                             (what & EBVO_FETCH_CSR) ? sizeof(int32_t) * (nL + 1) : 0,
                             (what & EBVO_FETCH_CSR) ? sizeof(int32_t) * np : 0,
                             (what & EBVO_FETCH_SIMS) ? sizeof(double) * 4 * np : 0,
                             (what & EBVO_FETCH_BEST) ? sizeof(double) * np : 0,
                             (what & EBVO_FETCH_KEEP) ? np : 0};
    size_t total = 0;
    for (int k = 0; k < 7; ++k)
    {
        s.fetch_off[k] = total;
        total += (sizes[k] + 63) & ~(size_t)63;
    }
    if (int rc_arena = ensure_arena(ctx, s, total))
        return rc_arena;
    const void *src[7] = {s.im[0].edges, s.im[1].edges, s.row_ptr.p, s.col_idx.p, s.sims.p, s.best.p, s.keep.p};
    char *base = static_cast<char *>(s.h_arena);
    // One copy stream for all slots: the pair is complete (the host has waited for it), so the copies need no ordering
    // against kernels, and on a stream of their own they never sit in front of another pair's kernels in a hardware queue.
    // The event marks the end of THIS slot's copies for ebvo_stereo_fetch_end and for the slot's next submission.
    if (!ctx->copy_stream)
        EBVO_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (int k = 0; k < 7; ++k)
        if (sizes[k])
            EBVO_HIP(ctx, hipMemcpyAsync(base + s.fetch_off[k], src[k], sizes[k], hipMemcpyDeviceToHost, ctx->copy_stream));
    EBVO_HIP(ctx, hipEventRecord(s.ev_rebind, ctx->copy_stream));
    s.fetch_what = what;
    s.fetch_compact = false;
    s.fetch_pending = true;
    return EBVO_OK;
}

extern "C" int ebvo_stereo_fetch_end(ebvo_ctx *ctx, int slot, ebvo_stereo_view *view)
{
    Slot *sp;
    if (!view || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    // (no have_run test: an asynchronous upload of the slot's NEXT images may already have been enqueued -- the copies started by
    // _begin read the result buffers, which only the next submission overwrites, and that clears fetch_what)
    if (s.in_flight || !s.fetch_what || s.fetch_compact)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (s.fetch_pending)
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_rebind));
    s.fetch_pending = false;
    const char *base = static_cast<const char *>(s.h_arena);
    const int what = s.fetch_what;
    memset(view, 0, sizeof *view);
    view->n_left = s.result.n_left;
    view->n_right = s.result.n_right;
    view->n_pairs = s.result.n_pairs;
    if (what & EBVO_FETCH_EDGES)
    {
        view->left = reinterpret_cast<const ebvo_edge *>(base + s.fetch_off[0]);
        view->right = reinterpret_cast<const ebvo_edge *>(base + s.fetch_off[1]);
    }
    if (what & EBVO_FETCH_CSR)
    {
        view->row_ptr = reinterpret_cast<const int32_t *>(base + s.fetch_off[2]);
        view->col_idx = reinterpret_cast<const int32_t *>(base + s.fetch_off[3]);
    }
    if (what & EBVO_FETCH_SIMS)
        view->sims = reinterpret_cast<const double *>(base + s.fetch_off[4]);
    if (what & EBVO_FETCH_BEST)
        view->best = reinterpret_cast<const double *>(base + s.fetch_off[5]);
    if (what & EBVO_FETCH_KEEP)
        view->keep = reinterpret_cast<const uint8_t *>(base + s.fetch_off[6]);
    return EBVO_OK;
}

// ---- compact results: what a consumer of the NCC stage reads, in fewer bytes (round 4) -------------------------------------
// The 32-byte ABI record of an edge carries its index (= its position in the list) and padding; (x, y) as 16 bytes and the
// orientation as a separate array on demand halve the edge traffic, and the keep flag of a pair is one bit.  best stays fp64.
namespace
{
__global__ __launch_bounds__(256) void pack_results_kernel(const ebvo_edge *__restrict__ L, int nL, const ebvo_edge *__restrict__ R,
                                                           int nR, const uint8_t *__restrict__ keep, int64_t np,
                                                           double2 *__restrict__ xyL, double2 *__restrict__ xyR,
                                                           double *__restrict__ thL, double *__restrict__ thR,
                                                           uint32_t *__restrict__ bits)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < nL; i += stride)
    {
        const ebvo_edge e = L[i];
        if (xyL) // (a selection of orientations without (x, y) has no room for them: they would land on the orientations)
            xyL[i] = make_double2(e.x, e.y);
        if (thL)
            thL[i] = e.theta;
    }
    for (int64_t i = t0; i < nR; i += stride)
    {
        const ebvo_edge e = R[i];
        if (xyR)
            xyR[i] = make_double2(e.x, e.y);
        if (thR)
            thR[i] = e.theta;
    }
    if (bits) // one 64-lane ballot = two words; every wave walks whole 64-pair groups (uniform trip count)
    {
        const int64_t groups = (np + 63) >> 6;
        const int64_t wave = t0 >> 6, waves = stride >> 6;
        const int lane = threadIdx.x & 63;
        for (int64_t g = wave; g < groups; g += waves)
        {
            const int64_t k = (g << 6) + lane;
            const unsigned long long m = __ballot(k < np && keep[k] != 0);
            if (lane == 0)
            {
                bits[2 * g] = (uint32_t)m;
                bits[2 * g + 1] = (uint32_t)(m >> 32);
            }
        }
    }
}
} // namespace

extern "C" int ebvo_stereo_fetch_compact_begin(ebvo_ctx *ctx, int slot, int what)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp) || what <= 0 || (what & ~EBVO_COMPACT_ALL))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_run || s.in_flight)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nL = (size_t)s.result.n_left, nR = (size_t)s.result.n_right, np = (size_t)s.result.n_pairs;
    s.fetch_packed = false;
    if (s.have_pack && (!(what & EBVO_COMPACT_THETA) || (s.params.reserved & EBVO_PAIR_PUSH_THETA)))
    {
        // the pair's own chain has packed the arrays (EBVO_PAIR_PACK): ONE copy of the block, sized by the actual counts
        const PackLayout lay = pack_layout(nL, nR, np, s.params.reserved & EBVO_PAIR_PUSH_THETA);
        if (int rc_arena = ensure_arena(ctx, s, lay.total))
            return rc_arena;
        if (!ctx->copy_stream)
            EBVO_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        EBVO_HIP(ctx, hipMemcpyAsync(s.h_arena, s.fetch_pack.p, lay.total, hipMemcpyDeviceToHost, ctx->copy_stream));
        EBVO_HIP(ctx, hipEventRecord(s.ev_rebind, ctx->copy_stream));
        s.fetch_what = what;
        s.fetch_compact = true;
        s.fetch_packed = true;
        s.fetch_packed_theta = (s.params.reserved & EBVO_PAIR_PUSH_THETA) != 0;
        s.fetch_result = s.result;
        s.fetch_pending = true;
        return EBVO_OK;
    }
    const size_t nwords = 2 * ((np + 63) >> 6);
    const bool xy = what & EBVO_COMPACT_XY, th = what & EBVO_COMPACT_THETA, kb = what & EBVO_COMPACT_KEEP_BITS;
    const size_t sizes[8] = {xy ? 16 * nL : 0, xy ? 16 * nR : 0, th ? 8 * nL : 0, th ? 8 * nR : 0,
                             (what & EBVO_COMPACT_CSR) ? sizeof(int32_t) * (nL + 1) : 0,
                             (what & EBVO_COMPACT_CSR) ? sizeof(int32_t) * np : 0,
                             (what & EBVO_COMPACT_BEST) ? sizeof(double) * np : 0, kb ? sizeof(uint32_t) * nwords : 0};
    size_t total = 0;
    for (int k = 0; k < 8; ++k)
    {
        s.fetch_off[k] = total;
        total += (sizes[k] + 63) & ~(size_t)63;
    }
    if (int rc_arena = ensure_arena(ctx, s, total))
        return rc_arena;
    if (!ctx->copy_stream)
        EBVO_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    // device staging of the packed arrays, laid out like the first four and the last array of the arena
    size_t poff[5], ptotal = 0;
    const size_t psizes[5] = {sizes[0], sizes[1], sizes[2], sizes[3], sizes[7]};
    for (int k = 0; k < 5; ++k)
    {
        poff[k] = ptotal;
        ptotal += (psizes[k] + 63) & ~(size_t)63;
    }
    // The staging below is fetch_pack, which also holds the block the chain of an EBVO_PAIR_PACK pair packed (one that asked
    // for THETA without EBVO_PAIR_PUSH_THETA lands here).  That block is overwritten now, in this path's own layout, so the
    // pair's later compact fetches take this path too instead of reading it with pack_layout.  (A staging buffer of its own
    // would keep their one copy, but costs every slot another buffer of the capacity's size.)
    s.have_pack = false;
    if (ptotal > s.fetch_pack.bytes && s.fetch_pending) // (re)allocation: the previous copies out of the old buffer must be over
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_rebind));
    int rc;
    if (ptotal && (rc = ebvo_grow(ctx, s, s.fetch_pack, ptotal)))
        return rc;
    char *pk = static_cast<char *>(s.fetch_pack.p);
    if (xy || th || kb)
    {
        const size_t work = nL > nR ? nL : nR;
        const size_t most = work > ((np + 63) >> 6) * 64 ? work : ((np + 63) >> 6) * 64;
        int blocks = (int)((most + 255) / 256);
        blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
        // the pair is complete (the host has waited for it) and the copy stream orders the kernel behind the previous copies
        // out of the staging buffer
        hipLaunchKernelGGL(pack_results_kernel, dim3(blocks), dim3(256), 0, ctx->copy_stream, (const ebvo_edge *)s.im[0].edges,
                           xy || th ? (int)nL : 0, (const ebvo_edge *)s.im[1].edges, xy || th ? (int)nR : 0,
                           (const uint8_t *)s.keep.p, kb ? (int64_t)np : 0, xy ? (double2 *)(pk + poff[0]) : nullptr,
                           xy ? (double2 *)(pk + poff[1]) : nullptr,
                           th ? (double *)(pk + poff[2]) : nullptr, th ? (double *)(pk + poff[3]) : nullptr,
                           kb ? (uint32_t *)(pk + poff[4]) : nullptr);
        EBVO_HIP(ctx, hipGetLastError());
    }
    const void *src[8] = {pk + poff[0], pk + poff[1], pk + poff[2], pk + poff[3], s.row_ptr.p, s.col_idx.p, s.best.p, pk + poff[4]};
    char *base = static_cast<char *>(s.h_arena);
    for (int k = 0; k < 8; ++k)
        if (sizes[k])
            EBVO_HIP(ctx, hipMemcpyAsync(base + s.fetch_off[k], src[k], sizes[k], hipMemcpyDeviceToHost, ctx->copy_stream));
    EBVO_HIP(ctx, hipEventRecord(s.ev_rebind, ctx->copy_stream));
    s.fetch_what = what;
    s.fetch_compact = true;
    s.fetch_pending = true;
    return EBVO_OK;
}

extern "C" int ebvo_stereo_fetch_compact_end(ebvo_ctx *ctx, int slot, ebvo_stereo_compact_view *view)
{
    Slot *sp;
    if (!view || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.in_flight || !s.fetch_what || !s.fetch_compact) // (see ebvo_stereo_fetch_end)
        return EBVO_ERR_STATE;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    if (s.fetch_pending)
        EBVO_HIP(ctx, hipEventSynchronize(s.ev_rebind));
    s.fetch_pending = false;
    const char *base = static_cast<const char *>(s.h_arena);
    const int what = s.fetch_what;
    if (s.fetch_packed)
    {
        const bool theta = s.fetch_packed_theta;
        const PackLayout lay = pack_layout((size_t)s.fetch_result.n_left, (size_t)s.fetch_result.n_right, (size_t)s.fetch_result.n_pairs, theta);
        fill_compact_view(view, base, lay, s.fetch_result, theta);
        if (!(what & EBVO_COMPACT_XY))
            view->left_xy = view->right_xy = nullptr;
        if (!(what & EBVO_COMPACT_THETA))
            view->left_theta = view->right_theta = nullptr;
        if (!(what & EBVO_COMPACT_CSR))
            view->row_ptr = view->col_idx = nullptr;
        if (!(what & EBVO_COMPACT_BEST))
            view->best = nullptr;
        if (!(what & EBVO_COMPACT_KEEP_BITS))
            view->keep_bits = nullptr;
        return EBVO_OK;
    }
    memset(view, 0, sizeof *view);
    view->n_left = s.result.n_left;
    view->n_right = s.result.n_right;
    view->n_pairs = s.result.n_pairs;
    view->n_matches = s.result.n_matches;
    if (what & EBVO_COMPACT_XY)
    {
        view->left_xy = reinterpret_cast<const double *>(base + s.fetch_off[0]);
        view->right_xy = reinterpret_cast<const double *>(base + s.fetch_off[1]);
    }
    if (what & EBVO_COMPACT_THETA)
    {
        view->left_theta = reinterpret_cast<const double *>(base + s.fetch_off[2]);
        view->right_theta = reinterpret_cast<const double *>(base + s.fetch_off[3]);
    }
    if (what & EBVO_COMPACT_CSR)
    {
        view->row_ptr = reinterpret_cast<const int32_t *>(base + s.fetch_off[4]);
        view->col_idx = reinterpret_cast<const int32_t *>(base + s.fetch_off[5]);
    }
    if (what & EBVO_COMPACT_BEST)
        view->best = reinterpret_cast<const double *>(base + s.fetch_off[6]);
    if (what & EBVO_COMPACT_KEEP_BITS)
        view->keep_bits = reinterpret_cast<const uint32_t *>(base + s.fetch_off[7]);
    return EBVO_OK;
}

extern "C" int ebvo_stereo_fetch(ebvo_ctx *ctx, ebvo_edge *left, ebvo_edge *right, int32_t *row_ptr,
                                 int32_t *col_idx, double *sims, double *best, uint8_t *keep, float *left_patches)
{
    return ebvo_stereo_fetch_slot(ctx, 0, left, right, row_ptr, col_idx, sims, best, keep, left_patches);
}

// ------------------------------------------------------------------------------------------
extern "C" int ebvo_profile_enable(ebvo_ctx *ctx, int on)
{
    if (!ctx)
        return EBVO_ERR_ARG;
    int rc = prof_drain(ctx);
    ctx->prof = on != 0;
    ctx->prof_every = on > 1 ? on : 1; // on = N > 1: sample every N-th pair submitted to the device pipeline
    ctx->prof_submits = 0;
    return rc;
}

extern "C" int ebvo_profile_reset(ebvo_ctx *ctx)
{
    if (!ctx)
        return EBVO_ERR_ARG;
    int rc = prof_drain(ctx);
    for (int k = 0; k < K_NUM; ++k)
    {
        ctx->prof_ms[k] = 0;
        ctx->prof_launches[k] = 0;
    }
    return rc;
}

extern "C" int ebvo_profile_get(ebvo_ctx *ctx, ebvo_kernel_time *out, int *n)
{
    if (!ctx || !out || !n)
        return EBVO_ERR_ARG;
    int rc = prof_drain(ctx);
    for (int k = 0; k < K_NUM; ++k)
    {
        out[k].name = g_kernel_names[k];
        out[k].ms = ctx->prof_ms[k];
        out[k].launches = ctx->prof_launches[k];
    }
    *n = K_NUM;
    return rc;
}

// ---- ground-truth evaluation from a disparity map (gt_kernels.hip) ------------------------------------------------------
extern "C" void ebvo_gt_default_params(ebvo_gt_params *p)
{
    if (!p)
        return;
    p->orient_gate_deg = 4.0; // src/Stereo_Matches.cpp:146
    p->pool_epi_thr = 0.5;    // :227
    p->pool_dist = 1.0;       // :228
    p->pool_orient_deg = 5.0; // :228
    p->tp_dist = 1.0;         // DIST_TO_GT_THRESH, include/definitions.h:42
}

static bool gt_params_ok(const ebvo_gt_params *p)
{
    return p->orient_gate_deg >= 0 && p->pool_epi_thr >= 0 && p->pool_dist >= 0 && p->pool_orient_deg >= 0 && p->tp_dist >= 0; // (false for NaN)
}

// The four doubles of a stage (:365-368) from the per-row (n, tp): plain sequential sums in row order, as std::accumulate
// forms them.  drop_empty: the rows of remove_empty_clusters (:1526).  The integer fields are filled too (host values).
static void gt_stage_doubles(const int32_t *rows, const uint8_t *focused, int nL, bool drop_empty, ebvo_gt_stage *st)
{
    int64_t n_rows = 0, nonempty = 0, with_tp = 0, sum_tp = 0, sum_n = 0;
    double acc_precision = 0.0, acc_pair = 0.0, acc_n = 0.0;
    for (int i = 0; i < nL; ++i)
    {
        if (!focused[i])
            continue;
        const int32_t n = rows[(size_t)i * 2], tp = rows[(size_t)i * 2 + 1];
        if (drop_empty && n == 0)
            continue;
        ++n_rows;
        if (n > 0)
        {
            ++nonempty;
            with_tp += tp > 0;
            sum_tp += tp;
            sum_n += n;
            const double q = static_cast<double>(tp) / static_cast<double>(n);
            acc_precision = acc_precision + q;
            acc_pair = acc_pair + q;
            acc_n = acc_n + static_cast<double>(n);
        }
        else
            acc_precision = acc_precision + 0.0;
    }
    st->rows = n_rows;
    st->nonempty = nonempty;
    st->rows_with_tp = with_tp;
    st->sum_tp = sum_tp;
    st->sum_n = sum_n;
    st->recall = static_cast<double>(with_tp) / static_cast<double>(n_rows);
    st->precision = acc_precision / static_cast<double>(n_rows);
    st->precision_pair = acc_pair / static_cast<double>(nonempty);
    st->ambiguity = acc_n / static_cast<double>(nonempty);
}

static int32_t *gt_stage_rows(Slot &s, int stage) { return (int32_t *)s.gt_rows.p + (size_t)stage * 2 * s.gt_nL; }
static unsigned long long *gt_stage_tot(Slot &s, int stage) { return (unsigned long long *)s.gt_tot.p + (size_t)stage * 8; }

extern "C" int ebvo_stereo_set_gt(ebvo_ctx *ctx, int slot, const float *disp, int h, int w, ptrdiff_t stride_elems,
                                  const ebvo_stereo_calib *calib, const ebvo_gt_params *params)
{
    Slot *sp;
    ebvo_gt_params P;
    ebvo_gt_default_params(&P);
    if (params)
        P = *params;
    // every argument and the slot's state are checked before anything of the slot changes
    if (!disp || !calib || !gt_params_ok(&P) || get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (!s.have_run || s.in_flight || s.fin_in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    if (h != s.cur_h || w != s.cur_w || stride_elems < w)
        return EBVO_ERR_ARG;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = drain_fetch(ctx, s)))
        return rc;
    const int nL = s.result.n_left, nR = s.result.n_right;
    const size_t nLz = (size_t)nL;
    s.gt_armed = false;
    s.gt_fin_enq = s.gt_fin_done = false;
    if ((rc = ebvo_grow(ctx, s, s.gt_disp, sizeof(float) * (size_t)h * w, false)) || (rc = ebvo_grow(ctx, s, s.gt_geom, sizeof(double) * 8 * (nLz + 1), false)) ||
        (rc = ebvo_grow(ctx, s, s.gt_flags, 2 * (nLz + 1), false)) || (rc = ebvo_grow(ctx, s, s.gt_boxes, gt_boxes_bytes(nR), false)) ||
        (rc = ebvo_grow(ctx, s, s.gt_pool_i32, sizeof(int32_t) * 2 * (nLz + 1), false)) ||
        (rc = ebvo_grow(ctx, s, s.gt_rows, sizeof(int32_t) * 2 * (nLz + 1) * EBVO_GT_NUM_STAGES, false)) ||
        (rc = ebvo_grow(ctx, s, s.gt_tot, sizeof(unsigned long long) * 8 * EBVO_GT_NUM_STAGES, false)))
        return rc;
    hipStream_t st = s.stream;
    s.gt_nL = nL;
    s.gt_params = P;
    s.gt_n_valid = s.gt_n_focused = 0;
    s.gt_n_pool = 0;
    s.gt_h_focused.assign(nLz, 0);
    s.gt_h_pool_rp.assign(nLz + 1, 0);
    double *gt_xy = (double *)s.gt_geom.p, *gl = gt_xy + 2 * nLz, *gr = gl + 3 * nLz;
    uint8_t *valid = (uint8_t *)s.gt_flags.p, *focused = valid + nLz;
    int32_t *cnt = (int32_t *)s.gt_pool_i32.p, *prp = cnt + nLz + 1;
    EBVO_HIP(ctx, hipMemsetAsync(s.gt_rows.p, 0, sizeof(int32_t) * 2 * (nLz + 1) * EBVO_GT_NUM_STAGES, st));
    EBVO_HIP(ctx, hipMemsetAsync(s.gt_tot.p, 0, sizeof(unsigned long long) * 8 * EBVO_GT_NUM_STAGES, st));
    if (nL > 0)
    {
        EBVO_HIP(ctx, hipMemcpy2DAsync(s.gt_disp.p, sizeof(float) * (size_t)w, disp, sizeof(float) * (size_t)stride_elems,
                                       sizeof(float) * (size_t)w, (size_t)h, hipMemcpyHostToDevice, st));
        std::vector<uint8_t> h_valid(nLz);
        if ((rc = gt_locate_enqueue(ctx, s, s.im[0].edges, nL, (const float *)s.gt_disp.p, h, w, w, calib, P.orient_gate_deg, valid,
                                    gt_xy, gl, gr)) ||
            (rc = gt_boxes_enqueue(ctx, s, s.im[1].edges, nR, s.gt_boxes.p)) ||
            (rc = gt_pool_enqueue(ctx, s, false, s.im[0].edges, nL, s.im[1].edges, nR, (const double *)s.lines.p, gt_xy, valid,
                                  s.gt_boxes.p, &P, cnt, nullptr, nullptr, nullptr)) ||
            (rc = ebvo_device_scan(ctx, s, cnt, prp, nL, nullptr, 1, nL + 1)))
            return rc;
        EBVO_HIP(ctx, hipMemcpyAsync(s.gt_h_pool_rp.data(), prp, sizeof(int32_t) * (nLz + 1), hipMemcpyDeviceToHost, st));
        EBVO_HIP(ctx, hipMemcpyAsync(h_valid.data(), valid, nLz, hipMemcpyDeviceToHost, st));
        EBVO_HIP(ctx, hipStreamSynchronize(st));
        const int64_t n_pool = s.gt_h_pool_rp[nLz];
        if ((rc = ebvo_grow(ctx, s, s.gt_pool_idx, sizeof(int32_t) * ((size_t)n_pool + 1), false)))
            return rc;
        if ((rc = gt_pool_enqueue(ctx, s, true, s.im[0].edges, nL, s.im[1].edges, nR, (const double *)s.lines.p, gt_xy, valid,
                                  s.gt_boxes.p, &P, cnt, prp, (int32_t *)s.gt_pool_idx.p, focused)) ||
            (rc = gt_census_enqueue(ctx, s, s.im[0].edges, nL, s.im[1].edges, nR, (const double *)s.lines.p, gt_xy, focused,
                                    s.gt_boxes.p, &s.params, P.tp_dist, gt_stage_rows(s, EBVO_GT_EPIPOLAR),
                                    gt_stage_rows(s, EBVO_GT_DISPARITY), gt_stage_rows(s, EBVO_GT_ORIENTATION))))
            return rc;
        for (int k = EBVO_GT_EPIPOLAR; k <= EBVO_GT_ORIENTATION; ++k)
            if ((rc = gt_totals_enqueue(ctx, s, gt_stage_rows(s, k), focused, nL, gt_stage_tot(s, k))))
                return rc;
        // the NCC stage of a chain without SIFT (:1427): the resident CSR with the run's keep flags
        if ((rc = gt_rows_enqueue(ctx, s, (const int32_t *)s.row_ptr.p, nullptr, (const int32_t *)s.col_idx.p, s.im[1].edges,
                                  (const uint8_t *)s.keep.p, gt_xy, focused, nL, P.tp_dist, gt_stage_rows(s, EBVO_GT_NCC),
                                  gt_stage_tot(s, EBVO_GT_NCC))))
            return rc;
        EBVO_HIP(ctx, hipMemcpyAsync(s.gt_h_focused.data(), focused, nLz, hipMemcpyDeviceToHost, st));
        EBVO_HIP(ctx, hipStreamSynchronize(st));
        for (size_t i = 0; i < nLz; ++i)
        {
            s.gt_n_valid += h_valid[i] != 0;
            s.gt_n_focused += s.gt_h_focused[i] != 0;
        }
        s.gt_n_pool = n_pool;
    }
    else
        EBVO_HIP(ctx, hipStreamSynchronize(st));
    s.gt_armed = true;
    return EBVO_OK;
}

static int gt_armed_slot(ebvo_ctx *ctx, int slot, Slot **out)
{
    if (get_slot(ctx, slot, out))
        return EBVO_ERR_ARG;
    Slot &s = **out;
    if (!s.gt_armed || !s.have_run || s.in_flight || s.fin_in_flight || s.tq_in_flight)
        return EBVO_ERR_STATE;
    return EBVO_OK;
}

extern "C" int ebvo_stereo_gt_size(ebvo_ctx *ctx, int slot, int32_t *n_valid, int32_t *n_focused, int64_t *n_pool)
{
    Slot *sp;
    if (int rc = gt_armed_slot(ctx, slot, &sp))
        return rc;
    if (n_valid)
        *n_valid = sp->gt_n_valid;
    if (n_focused)
        *n_focused = sp->gt_n_focused;
    if (n_pool)
        *n_pool = sp->gt_n_pool;
    return EBVO_OK;
}

extern "C" int ebvo_stereo_gt_fetch(ebvo_ctx *ctx, int slot, int32_t *focused_index, double *gt_xy, double *gamma_left,
                                    double *gamma_right, int32_t *pool_row_ptr, int32_t *pool_idx)
{
    Slot *sp;
    if (int rc = gt_armed_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nLz = (size_t)s.gt_nL;
    std::vector<double> geom;
    if ((gt_xy || gamma_left || gamma_right) && nLz)
    {
        geom.resize(8 * nLz);
        EBVO_HIP(ctx, hipMemcpyAsync(geom.data(), s.gt_geom.p, sizeof(double) * 8 * nLz, hipMemcpyDeviceToHost, s.stream));
    }
    if (pool_idx && s.gt_n_pool > 0) // rows that are not focused have an empty pool: the list is compact as it stands
        EBVO_HIP(ctx, hipMemcpyAsync(pool_idx, s.gt_pool_idx.p, sizeof(int32_t) * (size_t)s.gt_n_pool, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    size_t q = 0;
    for (size_t i = 0; i < nLz; ++i)
    {
        if (!s.gt_h_focused[i])
            continue;
        if (focused_index)
            focused_index[q] = (int32_t)i;
        if (pool_row_ptr)
            pool_row_ptr[q] = s.gt_h_pool_rp[i];
        if (gt_xy)
            for (int k = 0; k < 2; ++k)
                gt_xy[q * 2 + k] = geom[i * 2 + k];
        if (gamma_left)
            for (int k = 0; k < 3; ++k)
                gamma_left[q * 3 + k] = geom[2 * nLz + i * 3 + k];
        if (gamma_right)
            for (int k = 0; k < 3; ++k)
                gamma_right[q * 3 + k] = geom[5 * nLz + i * 3 + k];
        ++q;
    }
    if (pool_row_ptr)
        pool_row_ptr[q] = (int32_t)s.gt_n_pool;
    return EBVO_OK;
}

static bool gt_stage_present(const Slot &s, int stage)
{
    switch (stage)
    {
    case EBVO_GT_EPIPOLAR: case EBVO_GT_DISPARITY: case EBVO_GT_ORIENTATION: case EBVO_GT_NCC:
        return true;
    case EBVO_GT_SIFT: case EBVO_GT_BNB_SIFT:
        return s.gt_fin_done && s.gt_fin_sift;
    default:
        return s.gt_fin_done;
    }
}

extern "C" int ebvo_stereo_gt_stage_rows(ebvo_ctx *ctx, int slot, int stage, int32_t *rows_n_tp, int32_t cap_rows)
{
    Slot *sp;
    if (!rows_n_tp || stage < 0 || stage >= EBVO_GT_NUM_STAGES || cap_rows < 0)
        return EBVO_ERR_ARG;
    if (int rc = gt_armed_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    if (!gt_stage_present(s, stage))
        return EBVO_ERR_STATE;
    if (cap_rows < s.gt_nL)
    {
        ctx->last_error = "ebvo_stereo_gt_stage_rows: the slot has " + std::to_string(s.gt_nL) + " left edges";
        return EBVO_ERR_CAPACITY;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nLz = (size_t)s.gt_nL;
    if (!nLz)
        return EBVO_OK;
    EBVO_HIP(ctx, hipMemcpyAsync(rows_n_tp, gt_stage_rows(s, stage == EBVO_GT_FINAL ? EBVO_GT_BEST : stage), sizeof(int32_t) * 2 * nLz,
                                 hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    return EBVO_OK;
}

// One number, one source: a stage's integer totals are the device's reductions (gt_totals_kernel); the host walk that
// forms the four doubles counts the same rows, and a record is only returned when the two agree.  drop_empty: the rows
// of Final are Best's non-empty rows.
static int gt_totals_agree(ebvo_ctx *ctx, const ebvo_gt_stage &g, const unsigned long long *t, bool drop_empty)
{
    const int64_t dev[5] = {(int64_t)(drop_empty ? t[1] : t[0]), (int64_t)t[1], (int64_t)t[2], (int64_t)t[3], (int64_t)t[4]};
    if (dev[0] == g.rows && dev[1] == g.nonempty && dev[2] == g.rows_with_tp && dev[3] == g.sum_tp && dev[4] == g.sum_n)
        return EBVO_OK;
    ctx->last_error = "ground-truth stage " + std::to_string(g.stage) + ": the device totals differ from the per-row counts";
    return EBVO_ERR_HIP;
}

extern "C" int ebvo_stereo_gt_metrics(ebvo_ctx *ctx, int slot, ebvo_gt_stage *stages)
{
    Slot *sp;
    if (!stages)
        return EBVO_ERR_ARG;
    if (int rc = gt_armed_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nLz = (size_t)s.gt_nL;
    std::vector<int32_t> rows(2 * nLz * EBVO_GT_NUM_STAGES + 1);
    std::vector<unsigned long long> tot(8 * EBVO_GT_NUM_STAGES);
    if (nLz)
        EBVO_HIP(ctx, hipMemcpyAsync(rows.data(), s.gt_rows.p, sizeof(int32_t) * 2 * nLz * EBVO_GT_NUM_STAGES, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipMemcpyAsync(tot.data(), s.gt_tot.p, sizeof(unsigned long long) * 8 * EBVO_GT_NUM_STAGES, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    for (int k = 0; k < EBVO_GT_NUM_STAGES; ++k)
    {
        ebvo_gt_stage &g = stages[k];
        memset(&g, 0, sizeof g);
        g.stage = k;
        if (!gt_stage_present(s, k))
            continue;
        g.present = 1;
        const int src = k == EBVO_GT_FINAL ? EBVO_GT_BEST : k; // Final = Best without its empty rows (:1526)
        gt_stage_doubles(rows.data() + 2 * nLz * src, s.gt_h_focused.data(), s.gt_nL, k == EBVO_GT_FINAL, &g);
        if (int rc = gt_totals_agree(ctx, g, tot.data() + 8 * src, k == EBVO_GT_FINAL))
            return rc;
    }
    return EBVO_GT_NUM_STAGES;
}

extern "C" int ebvo_gt_locate(ebvo_ctx *ctx, const ebvo_edge *edges, int n, const float *disp, int h, int w, ptrdiff_t stride_elems,
                              const ebvo_stereo_calib *calib, const ebvo_gt_params *params, uint8_t *valid, double *gt_xy,
                              double *gamma_left, double *gamma_right)
{
    ebvo_gt_params P;
    ebvo_gt_default_params(&P);
    if (params)
        P = *params;
    if (!ctx || n < 0 || !disp || !calib || h <= 0 || w <= 0 || stride_elems < w || !gt_params_ok(&P) || (n > 0 && (!edges || !valid)))
        return EBVO_ERR_ARG;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    if (n == 0)
        return EBVO_OK;
    const size_t nz = (size_t)n;
    // edges, the eight doubles per edge, the map, the valid flags
    Carve L;
    const size_t o_e = L.take(sizeof(ebvo_edge) * nz), o_xy = L.take(sizeof(double) * 2 * nz), o_gl = L.take(sizeof(double) * 3 * nz),
                 o_gr = L.take(sizeof(double) * 3 * nz), o_disp = L.take(sizeof(float) * (size_t)h * w), o_valid = L.take(nz);
    if (hc.stage(L))
        return hc.rc;
    ebvo_edge *d_e = hc.at<ebvo_edge>(o_e);
    double *d_xy = hc.at<double>(o_xy), *d_gl = hc.at<double>(o_gl), *d_gr = hc.at<double>(o_gr);
    float *d_disp = hc.at<float>(o_disp);
    uint8_t *d_valid = hc.at<uint8_t>(o_valid);
    if (hc.up_rows(d_disp, disp, sizeof(float) * (size_t)w, sizeof(float) * (size_t)stride_elems, (size_t)h) ||
        hc.up(d_e, edges, sizeof(ebvo_edge) * nz))
        return hc.rc;
    if (int rc = gt_locate_enqueue(ctx, hc.slot(), d_e, n, d_disp, h, w, w, calib, P.orient_gate_deg, d_valid, d_xy, d_gl, d_gr))
        return rc;
    hc.down(valid, d_valid, nz);
    hc.down(gt_xy, d_xy, sizeof(double) * 2 * nz);
    hc.down(gamma_left, d_gl, sizeof(double) * 3 * nz);
    hc.down(gamma_right, d_gr, sizeof(double) * 3 * nz);
    return hc.finish();
}

static int host_stage_tail(HostCall &hc, const int32_t *d_rows, const unsigned long long *d_tot, int n, const uint8_t *on, bool temporal,
                           int32_t *n_tp, ebvo_gt_stage *stage_out); // defined with the temporal stages below

extern "C" int ebvo_gt_evaluate_rows(ebvo_ctx *ctx, const int32_t *row_ptr, const ebvo_edge *cand_edges, int nL, const uint8_t *focused,
                                     const double *gt_xy, double tp_dist, int32_t *n_tp, ebvo_gt_stage *stage_out)
{
    int64_t np = 0;
    if (!ctx || !stage_out || !(tp_dist >= 0) || check_csr(row_ptr, nL, &np) || (nL > 0 && (!focused || !gt_xy)) || (np > 0 && !cand_edges))
        return EBVO_ERR_ARG;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    memset(stage_out, 0, sizeof *stage_out);
    stage_out->present = 1;
    const size_t nLz = (size_t)nL, npz = (size_t)np;
    // candidates, gt_xy, the five totals, the (n, tp) rows, row_ptr, focused
    Carve L;
    const size_t o_cand = L.take(sizeof(ebvo_edge) * (npz + 1)), o_xy = L.take(sizeof(double) * 2 * (nLz + 1)),
                 o_tot = L.take(sizeof(unsigned long long) * 8), o_rows = L.take(sizeof(int32_t) * 2 * (nLz + 1)),
                 o_rp = L.take(sizeof(int32_t) * (nLz + 2)), o_f = L.take(nLz);
    if (hc.stage(L))
        return hc.rc;
    ebvo_edge *d_cand = hc.at<ebvo_edge>(o_cand);
    double *d_xy = hc.at<double>(o_xy);
    unsigned long long *d_tot = hc.at<unsigned long long>(o_tot);
    int32_t *d_rows = hc.at<int32_t>(o_rows), *d_rp = hc.at<int32_t>(o_rp);
    uint8_t *d_f = hc.at<uint8_t>(o_f);
    // without rows nothing below writes the totals
    if (hc.fill(d_tot, 0, sizeof(unsigned long long) * 8) || hc.up(d_cand, cand_edges, sizeof(ebvo_edge) * npz) ||
        hc.up(d_rp, row_ptr, sizeof(int32_t) * (nLz + 1)) || hc.up(d_xy, gt_xy, sizeof(double) * 2 * nLz) || hc.up(d_f, focused, nLz))
        return hc.rc;
    if (int rc = gt_rows_enqueue(ctx, hc.slot(), d_rp, d_cand, nullptr, nullptr, nullptr, d_xy, d_f, nL, tp_dist, d_rows, d_tot))
        return rc;
    return host_stage_tail(hc, d_rows, d_tot, nL, focused, /*temporal=*/false, n_tp, stage_out);
}

// ---- temporal ground truth from a relative pose (tgt_kernels.hip) -------------------------------------------------------
extern "C" void ebvo_tgt_default_params(ebvo_tgt_params *p)
{
    if (!p)
        return;
    p->orient_thr_deg = 10.0; // src/Temporal_Matches.cpp:67
    p->tp_dist = 2.0;         // DIST_TO_GT_THRESH_QUADS, include/definitions.h:43
    p->search_radius = 20.0;  // 15.0 + DIST_TO_GT_THRESH_QUADS + 3.0, :68
    p->img_margin = 10.0;     // :69
}

static bool tgt_params_ok(const ebvo_tgt_params *p)
{
    return p->orient_thr_deg >= 0 && p->tp_dist >= 0 && p->search_radius >= 0 && p->img_margin >= 0; // (false for NaN)
}

// static_cast<int>(std::ceil(radius / cell_size)) (include/Dataset.h:97), saturated as the temporal stage saturates its own
static int tgt_cell_radius(double radius, int cell)
{
    const double sr_d = ceil(radius / cell);
    return sr_d < (double)(1 << 30) ? (int)sr_d : (1 << 30);
}

// The four doubles of a stage (:259-282) from the per-row (n, tp), in KEYFRAME INDEX ORDER (the reference's order is that
// of its `out` vector, which OpenMP scheduling decides; this is its one-thread order).  No rows or no non-empty row: the
// four zeros of :274-278.
static void tgt_stage_doubles(const int32_t *rows, const uint8_t *on, int n_kf, ebvo_gt_stage *st)
{
    double recall_sum = 0.0, precision_sum = 0.0, ambiguity_sum = 0.0;
    int64_t n_rows = 0, matched = 0, with_tp = 0, sum_tp = 0, sum_n = 0;
    for (int i = 0; i < n_kf; ++i)
    {
        if (on && !on[i])
            continue;
        const int32_t n = rows[(size_t)i * 2], tp = rows[(size_t)i * 2 + 1];
        recall_sum += (tp >= 1) ? 1.0 : 0.0;
        precision_sum += (n == 0) ? 0.0 : (static_cast<double>(tp) / static_cast<double>(n));
        ambiguity_sum += static_cast<double>(n);
        ++n_rows;
        matched += n > 0;
        with_tp += tp > 0;
        sum_tp += tp;
        sum_n += n;
    }
    st->rows = n_rows;
    st->nonempty = matched;
    st->rows_with_tp = with_tp;
    st->sum_tp = sum_tp;
    st->sum_n = sum_n;
    st->recall = st->precision = st->precision_pair = st->ambiguity = 0.0;
    if (n_rows == 0 || matched == 0)
        return;
    st->recall = recall_sum / static_cast<double>(n_rows);
    st->precision = precision_sum / static_cast<double>(matched);
    st->precision_pair = st->precision;
    st->ambiguity = (ambiguity_sum / static_cast<double>(matched)) - 1.0;
}

// the slot's temporal match is complete, idle and still belongs to the stored keyframe
static int tgt_matched_slot(ebvo_ctx *ctx, int slot, Slot **out)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.tq_n < 0 || !s.have_final || s.in_flight || s.fin_in_flight || s.tq_in_flight || s.tq_kf_gen != ctx->kf_gen)
    {
        ctx->last_error = s.in_flight || s.fin_in_flight || s.tq_in_flight ? "the slot has work in flight (wait for it first)"
                          : s.tq_n < 0 || !s.have_final                    ? "the slot holds no temporal match (ebvo_temporal_match first)"
                                                         : "the keyframe was replaced since the slot's quads were matched";
        return EBVO_ERR_STATE;
    }
    *out = sp;
    return EBVO_OK;
}

static int tgt_armed_slot(ebvo_ctx *ctx, int slot, Slot **out)
{
    if (int rc = tgt_matched_slot(ctx, slot, out))
        return rc;
    if (!(*out)->tgt_armed)
    {
        ctx->last_error = "the slot is not armed (ebvo_temporal_set_gt after ebvo_temporal_match)";
        return EBVO_ERR_STATE;
    }
    return EBVO_OK;
}

// the stages the slot's match leaves behind: the position of their (n, tp) rows and totals.  The three of every match come
// first; a match that kept its trail (ebvo_temporal_keep_stages) adds the grid stage and, with stages = 1, the four interior
// lists behind them.
static int tgt_stage_pos(const Slot &s, int stage)
{
    if (stage == EBVO_TGT_ORIENTATION)
        return 0;
    if (stage == EBVO_TGT_NCC)
        return 1;
    if (stage == EBVO_TGT_CLUSTER && s.tq_final.n >= 0)
        return 2;
    if (stage == EBVO_TGT_GRID && s.tq_trail.on)
        return 3;
    if (stage >= EBVO_TGT_SIFT && stage <= EBVO_TGT_REFINE && s.tq_trail.on && s.tq_trail.lists)
        return 4 + (stage - EBVO_TGT_SIFT);
    return -1;
}

static int tgt_positions(const Slot &s)
{
    return s.tq_trail.on ? 8 : 3;
}

// host prefix of the per-row counts (they come to the host for the sizes anyway); false: more quads than an int32 row offset holds
static bool tgt_row_offsets(const std::vector<int32_t> &cnt, int n_kf, std::vector<int32_t> &rp, int32_t *n_rows)
{
    int64_t run = 0;
    int32_t rows = 0;
    rp.resize((size_t)n_kf + 1);
    for (int i = 0; i < n_kf; ++i)
    {
        rp[i] = (int32_t)run;
        run += cnt[i];
        rows += cnt[i] > 0;
        if (run > INT32_MAX)
            return false;
    }
    rp[n_kf] = (int32_t)run;
    *n_rows = rows;
    return true;
}

static bool tgt_pose_ok(const double *R, const double *t, const ebvo_stereo_calib *calib)
{
    if (!R || !t || !calib)
        return false;
    for (int k = 0; k < 9; ++k)
        if (std::isnan(R[k]) || std::isnan(calib->K_left[k]) || std::isnan(calib->K_right[k]) || std::isnan(calib->R21[k]))
            return false;
    for (int k = 0; k < 3; ++k)
        if (std::isnan(t[k]) || std::isnan(calib->T21[k]))
            return false;
    return true;
}

extern "C" int ebvo_temporal_set_gt(ebvo_ctx *ctx, int slot, const double R[9], const double t[3], const ebvo_stereo_calib *calib,
                                    const ebvo_tgt_params *params, const double *kf_gamma, const uint8_t *kf_is_tp)
{
    ebvo_tgt_params P;
    ebvo_tgt_default_params(&P);
    if (params)
        P = *params;
    if (!ctx || !tgt_pose_ok(R, t, calib) || !tgt_params_ok(&P))
        return EBVO_ERR_ARG;
    Slot *sp;
    if (int rc = tgt_matched_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    s.tgt_armed = false;
    const int n_kf = s.tq_n_kf, n_cf = s.n_final;
    const size_t nz = (size_t)n_kf, nq = (size_t)s.tq_n, nfin = (size_t)(s.tq_final.n > 0 ? s.tq_final.n : 0);
    const Slot::TqTrail &T = s.tq_trail;
    const size_t npos = (size_t)tgt_positions(s);
    // flag segments: candidates, candidates (the NCC stage reads them through keep), final quads, then the trail's four lists
    {
        const int64_t n_of[EBVO_TGT_NUM_STAGES] = {0, (int64_t)nq, (int64_t)nq, T.n[0], T.n[1], T.n[2], T.n[3], (int64_t)nfin};
        const int order[EBVO_TGT_NUM_STAGES] = {EBVO_TGT_ORIENTATION, EBVO_TGT_NCC, EBVO_TGT_CLUSTER, EBVO_TGT_GRID, EBVO_TGT_SIFT,
                                                EBVO_TGT_BNB_NCC, EBVO_TGT_BNB_SIFT, EBVO_TGT_REFINE};
        size_t run = 0;
        for (int k : order)
        {
            s.tgt_flag_off[k] = run;
            s.tgt_flag_n[k] = tgt_stage_pos(s, k) >= 0 ? n_of[k] : 0;
            run += (size_t)s.tgt_flag_n[k];
        }
    }
    const size_t n_flags = s.tgt_flag_off[EBVO_TGT_REFINE] + (size_t)s.tgt_flag_n[EBVO_TGT_REFINE];
    int rc;
    if ((rc = ebvo_grow(ctx, s, s.tgt_geom, sizeof(double) * 9 * nz + 64, false)) || (rc = ebvo_grow(ctx, s, s.tgt_u8, 3 * nz + 64, false)) ||
        (rc = ebvo_grow(ctx, s, s.tgt_i32, sizeof(int32_t) * 2 * (nz + 1), false)) ||
        (rc = ebvo_grow(ctx, s, s.tgt_rows, sizeof(int32_t) * 2 * npos * nz + 64, false)) || (rc = ebvo_grow(ctx, s, s.tgt_flags, n_flags + 64, false)) ||
        (rc = ebvo_grow(ctx, s, s.tgt_tot, sizeof(unsigned long long) * 8 * npos, false)))
        return rc;
    hipStream_t st = s.stream;
    double *pl = (double *)s.tgt_geom.p, *pr = pl + 2 * nz, *ol = pr + 2 * nz, *orr = ol + nz, *gamma = orr + nz;
    uint8_t *in = (uint8_t *)s.tgt_u8.p, *on = in + nz, *is_tp = on + nz;
    int32_t *cnt = (int32_t *)s.tgt_i32.p, *rp = cnt + nz + 1;
    EBVO_HIP(ctx, hipMemsetAsync(s.tgt_tot.p, 0, sizeof(unsigned long long) * 8 * npos, st));
    EBVO_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(int32_t) * 2 * (nz + 1), st));
    if (nz)
    {
        EBVO_HIP(ctx, hipMemsetAsync(s.tgt_rows.p, 0, sizeof(int32_t) * 2 * npos * nz, st));
        EBVO_HIP(ctx, hipMemsetAsync(in, 0, 3 * nz, st));
        if (kf_gamma)
            EBVO_HIP(ctx, hipMemcpyAsync(gamma, kf_gamma, sizeof(double) * 3 * nz, hipMemcpyHostToDevice, st));
        if (kf_is_tp)
            EBVO_HIP(ctx, hipMemcpyAsync(is_tp, kf_is_tp, nz, hipMemcpyHostToDevice, st));
    }
    std::vector<int32_t> h_cnt(nz + 1, 0), h_rp;
    int32_t n_rows = 0;
    const ebvo_edge *cfL = nullptr, *cfR = nullptr;
    const bool walk = n_kf > 0 && n_cf > 0 && !s.tq_empty;
    if (n_kf > 0 &&
        (rc = tgt_project_enqueue(ctx, s, ctx->kf_L, ctx->kf_R, kf_gamma ? gamma : nullptr, n_kf, R, t, calib, P.img_margin, s.cur_w,
                                  s.cur_h, in, pl, pr, ol, orr)))
        return rc;
    // the current-frame grid of the slot's own match (temporal_stage0_enqueue built it with tq_params.cell_size and nothing
    // has written it since): read, never written
    const int cell = s.tq_params.cell_size, gw = (int)(((int64_t)s.cur_w + cell - 1) / cell), gh = (int)(((int64_t)s.cur_h + cell - 1) / cell);
    const int sr = tgt_cell_radius(P.search_radius, cell);
    if (walk)
    {
        final_mates(s, &cfL, &cfR);
        if ((rc = tgt_veridical_enqueue(ctx, s, n_kf, in, pl, pr, ol, orr, cfL, cfR, s.tq_cells.p, n_cf, cell, sr, gw, gh, P.tp_dist,
                                        P.orient_thr_deg, kf_is_tp ? is_tp : nullptr, cnt, nullptr, nullptr, 0, nullptr)))
            return rc;
        EBVO_HIP(ctx, hipMemcpyAsync(h_cnt.data(), cnt, sizeof(int32_t) * nz, hipMemcpyDeviceToHost, st));
    }
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    if (!tgt_row_offsets(h_cnt, n_kf, h_rp, &n_rows))
    {
        ctx->last_error = "more veridical quads than a 32-bit row offset holds";
        return EBVO_ERR_CAPACITY;
    }
    const int64_t n_ver = h_rp[n_kf];
    if ((rc = ebvo_grow(ctx, s, s.tgt_idx, sizeof(int32_t) * (size_t)(n_ver + 1), false)))
        return rc;
    s.tgt_h_on.assign(nz, 0);
    if (walk) // otherwise the offsets are the zeros written above; h_rp outlives the copy through the synchronise below
    {
        EBVO_HIP(ctx, hipMemcpyAsync(rp, h_rp.data(), sizeof(int32_t) * (nz + 1), hipMemcpyHostToDevice, st));
        if ((rc = tgt_veridical_enqueue(ctx, s, n_kf, in, pl, pr, ol, orr, cfL, cfR, s.tq_cells.p, n_cf, cell, sr, gw, gh, P.tp_dist,
                                        P.orient_thr_deg, kf_is_tp ? is_tp : nullptr, nullptr, rp, (int32_t *)s.tgt_idx.p, n_ver, on)))
            return rc;
        EBVO_HIP(ctx, hipMemcpyAsync(s.tgt_h_on.data(), on, nz, hipMemcpyDeviceToHost, st));
        // the three lists the match left behind: candidates, candidates with keep, final quads
        const size_t nk1 = nz + 1, ncz = (size_t)n_cf;
        const int32_t *q_rp = (const int32_t *)s.tq_i32.p + nk1, *q_col = (const int32_t *)s.tq_cols.p;
        const uint8_t *q_keep = (const uint8_t *)s.tq_u8.p + ((2 * ncz + 63) & ~(size_t)63);
        int32_t *rows = (int32_t *)s.tgt_rows.p;
        uint8_t *flags = (uint8_t *)s.tgt_flags.p;
        unsigned long long *tot = (unsigned long long *)s.tgt_tot.p;
        if (s.tq_n > 0 &&
            ((rc = tgt_rows_enqueue(ctx, s, q_rp, nullptr, nullptr, q_col, cfL, cfR, nullptr, pl, pr, on, n_kf, s.tq_n, P.tp_dist, rows,
                                    flags, tot)) ||
             (rc = tgt_rows_enqueue(ctx, s, q_rp, nullptr, nullptr, q_col, cfL, cfR, q_keep, pl, pr, on, n_kf, s.tq_n, P.tp_dist,
                                    rows + 2 * nz, flags + nq, tot + 8))))
            return rc;
        if (s.tq_n == 0) // empty lists: the rows still count (gt_totals over zeroed (n, tp))
            if ((rc = gt_totals_enqueue(ctx, s, rows, on, n_kf, tot)) || (rc = gt_totals_enqueue(ctx, s, rows + 2 * nz, on, n_kf, tot + 8)))
                return rc;
        if (s.tq_final.n >= 0)
        {
            const Slot::TqFinal &F = s.tq_final;
            if (F.n > 0)
                rc = tgt_rows_enqueue(ctx, s, F.rp, F.L, F.R, nullptr, nullptr, nullptr, nullptr, pl, pr, on, n_kf, F.n, P.tp_dist,
                                      rows + 4 * nz, flags + 2 * nq, tot + 16);
            else
                rc = gt_totals_enqueue(ctx, s, rows + 4 * nz, on, n_kf, tot + 16);
            if (rc)
                return rc;
        }
        if (T.on)
        {
            // "Location Proximity" on the match's own grid and radius, then the trail's lists: mates by index, the last one
            // by its refined centres
            int pos = tgt_stage_pos(s, EBVO_TGT_GRID);
            // (a match made under a pose prior searched around the prior's projections: those cells are counted)
            const TemporalPrior prior_q = s.tq_prior.on ? temporal_prior_view(s) : TemporalPrior{};
            if ((rc = tgt_grid_rows_enqueue(ctx, s, ctx->kf_L, ctx->kf_R, n_kf, cfL, cfR, s.tq_cells.p, n_cf, cell,
                                            tgt_cell_radius(s.tq_params.grid_radius, cell), gw, gh, on, pl, pr, P.tp_dist,
                                            rows + 2 * nz * pos, tot + 8 * pos, s.tq_prior.on ? &prior_q : nullptr)))
                return rc;
            for (int k = EBVO_TGT_SIFT; k <= EBVO_TGT_REFINE && T.lists; ++k)
            {
                const int t = k - EBVO_TGT_SIFT;
                pos = tgt_stage_pos(s, k);
                const bool refined = k == EBVO_TGT_REFINE;
                if (T.n[t] > 0)
                    rc = tgt_rows_enqueue(ctx, s, T.rp[t], refined ? T.cenL : nullptr, refined ? T.cenR : nullptr, refined ? nullptr : T.cf[t],
                                          cfL, cfR, nullptr, pl, pr, on, n_kf, T.n[t], P.tp_dist, rows + 2 * nz * pos,
                                          flags + s.tgt_flag_off[k], tot + 8 * pos);
                else
                    rc = gt_totals_enqueue(ctx, s, rows + 2 * nz * pos, on, n_kf, tot + 8 * pos);
                if (rc)
                    return rc;
            }
        }
        EBVO_HIP(ctx, hipStreamSynchronize(st));
    }
    s.tgt_n_kf = n_kf;
    s.tgt_n_rows = n_rows;
    s.tgt_n_ver = n_ver;
    s.tgt_armed = true;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_gt_size(ebvo_ctx *ctx, int slot, int32_t *n_kf, int32_t *n_rows, int64_t *n_veridical)
{
    Slot *sp;
    if (int rc = tgt_armed_slot(ctx, slot, &sp))
        return rc;
    if (n_kf)
        *n_kf = sp->tgt_n_kf;
    if (n_rows)
        *n_rows = sp->tgt_n_rows;
    if (n_veridical)
        *n_veridical = sp->tgt_n_ver;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_gt_fetch(ebvo_ctx *ctx, int slot, uint8_t *in_image, double *proj_left, double *proj_right,
                                      double *orient_left, double *orient_right, int32_t *ver_row_ptr, int32_t *ver_idx)
{
    Slot *sp;
    if (int rc = tgt_armed_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nz = (size_t)s.tgt_n_kf;
    hipStream_t st = s.stream;
    const double *pl = (const double *)s.tgt_geom.p, *pr = pl + 2 * nz, *ol = pr + 2 * nz, *orr = ol + nz;
    if (ver_row_ptr)
        EBVO_HIP(ctx, hipMemcpyAsync(ver_row_ptr, (const int32_t *)s.tgt_i32.p + nz + 1, sizeof(int32_t) * (nz + 1), hipMemcpyDeviceToHost, st));
    if (nz)
    {
        const struct
        {
            void *dst;
            const void *src;
            size_t bytes;
        } copies[] = {{in_image, s.tgt_u8.p, nz}, {proj_left, pl, sizeof(double) * 2 * nz}, {proj_right, pr, sizeof(double) * 2 * nz},
                      {orient_left, ol, sizeof(double) * nz}, {orient_right, orr, sizeof(double) * nz}};
        for (const auto &c : copies)
            if (c.dst)
                EBVO_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, st));
    }
    if (ver_idx && s.tgt_n_ver > 0)
        EBVO_HIP(ctx, hipMemcpyAsync(ver_idx, s.tgt_idx.p, sizeof(int32_t) * (size_t)s.tgt_n_ver, hipMemcpyDeviceToHost, st));
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    return EBVO_OK;
}

// One number, one source, as gt_totals_agree: the device's integer totals and the host walk count the same rows
static int tgt_totals_agree(ebvo_ctx *ctx, const ebvo_gt_stage &g, const unsigned long long *t)
{
    if ((int64_t)t[0] == g.rows && (int64_t)t[1] == g.nonempty && (int64_t)t[2] == g.rows_with_tp && (int64_t)t[3] == g.sum_tp &&
        (int64_t)t[4] == g.sum_n)
        return EBVO_OK;
    ctx->last_error = "temporal ground-truth stage " + std::to_string(g.stage) + ": the device totals differ from the per-row counts";
    return EBVO_ERR_HIP;
}

// The tail of a host-array stage call: the (n, tp) rows and the five totals come back, the call ends, the stage's doubles are
// formed from the rows (the stereo stage's or the temporal one's, over the rows that `on` keeps) and checked against the
// totals.  The locals the copies write into are safe here: finish() waits on every path before they go.
static int host_stage_tail(HostCall &hc, const int32_t *d_rows, const unsigned long long *d_tot, int n, const uint8_t *on, bool temporal,
                           int32_t *n_tp, ebvo_gt_stage *stage_out)
{
    const size_t nz = (size_t)n;
    std::vector<int32_t> rows(2 * nz + 1);
    unsigned long long tot[5] = {0, 0, 0, 0, 0};
    hc.down(rows.data(), d_rows, sizeof(int32_t) * 2 * nz);
    hc.down(tot, d_tot, sizeof tot);
    if (hc.finish())
        return hc.rc;
    if (temporal)
        tgt_stage_doubles(rows.data(), on, n, stage_out);
    else
        gt_stage_doubles(rows.data(), on, n, false, stage_out);
    if (int rc = temporal ? tgt_totals_agree(hc.ctx, *stage_out, tot) : gt_totals_agree(hc.ctx, *stage_out, tot, false))
        return rc;
    if (n_tp && n)
        memcpy(n_tp, rows.data(), sizeof(int32_t) * 2 * nz);
    return EBVO_OK;
}

extern "C" int ebvo_temporal_gt_metrics(ebvo_ctx *ctx, int slot, ebvo_gt_stage *stages)
{
    Slot *sp;
    if (!stages)
        return EBVO_ERR_ARG;
    if (int rc = tgt_armed_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nz = (size_t)s.tgt_n_kf;
    const size_t npos = (size_t)tgt_positions(s);
    std::vector<int32_t> rows(2 * npos * nz + 1);
    unsigned long long tot[8 * 8];
    if (nz)
        EBVO_HIP(ctx, hipMemcpyAsync(rows.data(), s.tgt_rows.p, sizeof(int32_t) * 2 * npos * nz, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipMemcpyAsync(tot, s.tgt_tot.p, sizeof(unsigned long long) * 8 * npos, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    for (int k = 0; k < EBVO_TGT_NUM_STAGES; ++k)
    {
        ebvo_gt_stage &g = stages[k];
        memset(&g, 0, sizeof g);
        g.stage = k;
        const int pos = tgt_stage_pos(s, k);
        if (pos < 0)
            continue;
        g.present = 1;
        tgt_stage_doubles(rows.data() + 2 * nz * pos, s.tgt_h_on.data(), s.tgt_n_kf, &g);
        if (int rc = tgt_totals_agree(ctx, g, tot + 8 * pos))
            return rc;
    }
    return EBVO_TGT_NUM_STAGES;
}

extern "C" int ebvo_temporal_gt_flags(ebvo_ctx *ctx, int slot, int stage, uint8_t *is_tp)
{
    Slot *sp;
    if (stage < 0 || stage >= EBVO_TGT_NUM_STAGES)
        return EBVO_ERR_ARG;
    if (int rc = tgt_armed_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    const int pos = tgt_stage_pos(s, stage);
    if (pos < 0 || stage == EBVO_TGT_GRID)
    {
        ctx->last_error = pos < 0 ? "the slot's match did not form this stage"
                                  : "the grid stage keeps no list of quads (ebvo_temporal_gt_stage_rows has its per-row counts)";
        return EBVO_ERR_STATE;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)s.tgt_flag_n[stage];
    if (!n || !is_tp)
        return EBVO_OK;
    const bool walked = s.tgt_n_kf > 0 && s.n_final > 0 && !s.tq_empty;
    if (!walked)
    {
        memset(is_tp, 0, n);
        return EBVO_OK;
    }
    const uint8_t *flags = (const uint8_t *)s.tgt_flags.p + s.tgt_flag_off[stage];
    if (stage != EBVO_TGT_NCC)
    {
        EBVO_HIP(ctx, hipMemcpyAsync(is_tp, flags, n, hipMemcpyDeviceToHost, s.stream));
        EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
        return EBVO_OK;
    }
    // the NCC stage's list is the candidates with keep: compacted here, in candidate order
    std::vector<uint8_t> f(n), keep(n);
    const uint8_t *q_keep = (const uint8_t *)s.tq_u8.p + ((2 * (size_t)s.n_final + 63) & ~(size_t)63);
    EBVO_HIP(ctx, hipMemcpyAsync(f.data(), flags, n, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipMemcpyAsync(keep.data(), q_keep, n, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    size_t o = 0;
    for (size_t k = 0; k < n; ++k)
        if (keep[k])
            is_tp[o++] = f[k];
    return EBVO_OK;
}

extern "C" int ebvo_temporal_gt_stage_rows(ebvo_ctx *ctx, int slot, int stage, int32_t *rows_n_tp, int32_t cap_rows)
{
    Slot *sp;
    if (!rows_n_tp || stage < 0 || stage >= EBVO_TGT_NUM_STAGES || cap_rows < 0)
        return EBVO_ERR_ARG;
    if (int rc = tgt_armed_slot(ctx, slot, &sp))
        return rc;
    Slot &s = *sp;
    const int pos = tgt_stage_pos(s, stage);
    if (pos < 0)
    {
        ctx->last_error = "the slot's match did not form this stage";
        return EBVO_ERR_STATE;
    }
    if (cap_rows < s.tgt_n_kf)
    {
        ctx->last_error = "ebvo_temporal_gt_stage_rows: the slot has " + std::to_string(s.tgt_n_kf) + " keyframe mates";
        return EBVO_ERR_CAPACITY;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nz = (size_t)s.tgt_n_kf;
    if (!nz)
        return EBVO_OK;
    EBVO_HIP(ctx, hipMemcpyAsync(rows_n_tp, (const int32_t *)s.tgt_rows.p + 2 * nz * (size_t)pos, sizeof(int32_t) * 2 * nz,
                                 hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    return EBVO_OK;
}

// the interior stage of a match that kept its trail: 0 .. 3, or a negative status with the last error set
static int tgt_trail_stage(ebvo_ctx *ctx, int slot, int stage, Slot **out)
{
    if (stage < EBVO_TGT_SIFT || stage > EBVO_TGT_REFINE)
    {
        if (ctx)
            ctx->last_error = stage == EBVO_TGT_ORIENTATION || stage == EBVO_TGT_NCC
                                  ? "this stage's list is what ebvo_temporal_fetch returns (the NCC stage: its quads with keep)"
                              : stage == EBVO_TGT_CLUSTER ? "this stage's list is what ebvo_temporal_fetch_final returns"
                              : stage == EBVO_TGT_GRID
                                  ? "the grid stage keeps no list of quads (ebvo_temporal_gt_stage_rows has its per-row counts)"
                                  : "no such stage";
        return EBVO_ERR_ARG;
    }
    if (!ctx)
        return EBVO_ERR_ARG;
    if (int rc = tgt_matched_slot(ctx, slot, out))
        return rc;
    if (!(*out)->tq_trail.on || !(*out)->tq_trail.lists)
    {
        ctx->last_error = "the slot's match kept no stage trail (ebvo_temporal_keep_stages, then a match with stages = 1)";
        return EBVO_ERR_STATE;
    }
    return stage - EBVO_TGT_SIFT;
}

extern "C" int ebvo_temporal_stage_size(ebvo_ctx *ctx, int slot, int stage, int64_t *n)
{
    Slot *sp;
    const int t = tgt_trail_stage(ctx, slot, stage, &sp);
    if (t < 0)
        return t;
    if (n)
        *n = sp->tq_trail.n[t];
    return EBVO_OK;
}

extern "C" int ebvo_temporal_fetch_stage(ebvo_ctx *ctx, int slot, int stage, int32_t *row_ptr, int32_t *cf_index, ebvo_edge *left,
                                         ebvo_edge *right)
{
    Slot *sp;
    const int t = tgt_trail_stage(ctx, slot, stage, &sp);
    if (t < 0)
        return t;
    Slot &s = *sp;
    const Slot::TqTrail &T = s.tq_trail;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = s.stream;
    const size_t n = (size_t)T.n[t], ncz = (size_t)s.n_final;
    if (row_ptr)
        EBVO_HIP(ctx, hipMemcpyAsync(row_ptr, T.rp[t], sizeof(int32_t) * ((size_t)s.tq_n_kf + 1), hipMemcpyDeviceToHost, st));
    std::vector<int32_t> cf(n);
    std::vector<ebvo_edge> mates[2];
    const bool refined = stage == EBVO_TGT_REFINE, gather = !refined && (left || right);
    if (n)
    {
        EBVO_HIP(ctx, hipMemcpyAsync(cf.data(), T.cf[t], sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        if (refined)
        {
            if (left)
                EBVO_HIP(ctx, hipMemcpyAsync(left, T.cenL, sizeof(ebvo_edge) * n, hipMemcpyDeviceToHost, st));
            if (right)
                EBVO_HIP(ctx, hipMemcpyAsync(right, T.cenR, sizeof(ebvo_edge) * n, hipMemcpyDeviceToHost, st));
        }
        else if (gather)
        {
            // before the refinement the centres of a quad are its current-frame mate's edges
            const ebvo_edge *cfL, *cfR;
            final_mates(s, &cfL, &cfR);
            mates[0].resize(ncz);
            mates[1].resize(ncz);
            EBVO_HIP(ctx, hipMemcpyAsync(mates[0].data(), cfL, sizeof(ebvo_edge) * ncz, hipMemcpyDeviceToHost, st));
            EBVO_HIP(ctx, hipMemcpyAsync(mates[1].data(), cfR, sizeof(ebvo_edge) * ncz, hipMemcpyDeviceToHost, st));
        }
    }
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    for (size_t k = 0; k < n; ++k)
    {
        if (cf_index)
            cf_index[k] = cf[k];
        if (gather && left)
            left[k] = mates[0][(size_t)cf[k]];
        if (gather && right)
            right[k] = mates[1][(size_t)cf[k]];
    }
    return EBVO_OK;
}

extern "C" int ebvo_tgt_grid_rows(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const ebvo_edge *cf_left,
                                  const ebvo_edge *cf_right, int n_cf, int img_w, int img_h, int cell_size, double grid_radius,
                                  const uint8_t *row_on, const double *proj_left, const double *proj_right, double tp_dist,
                                  int32_t *n_tp, ebvo_gt_stage *stage_out)
{
    if (!ctx || !stage_out || n_kf < 0 || n_cf < 0 || img_w < 1 || img_h < 1 || cell_size < 1 ||
        !(grid_radius >= 0 && std::isfinite(grid_radius)) || !(tp_dist >= 0) ||
        (n_kf > 0 && (!kf_left || !kf_right || !proj_left || !proj_right)) || (n_cf > 0 && (!cf_left || !cf_right)))
        return EBVO_ERR_ARG;
    const int64_t gw64 = ((int64_t)img_w + cell_size - 1) / cell_size, gh64 = ((int64_t)img_h + cell_size - 1) / cell_size;
    if (gw64 * gh64 > (1 << 26) || gw64 > 30000 || gh64 > 30000) // the cells of a mate are 16-bit
        return EBVO_ERR_ARG;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    memset(stage_out, 0, sizeof *stage_out);
    stage_out->stage = EBVO_TGT_GRID;
    stage_out->present = 1;
    const int gw = (int)gw64, gh = (int)gh64;
    const size_t nz = (size_t)n_kf, ncz = (size_t)n_cf, eb = sizeof(ebvo_edge);
    // the four mate lists, both projections, the totals, the (n, tp) rows, row_on, the grid
    Carve L;
    const size_t o_kfL = L.take(eb * nz), o_kfR = L.take(eb * nz), o_cfL = L.take(eb * ncz), o_cfR = L.take(eb * ncz),
                 o_pl = L.take(sizeof(double) * 2 * nz), o_pr = L.take(sizeof(double) * 2 * nz), o_tot = L.take(sizeof(unsigned long long) * 8),
                 o_rows = L.take(sizeof(int32_t) * 2 * (nz + 1)), o_on = L.take(nz), o_grid = L.take(match_temporal_grid_bytes(n_cf, gw * gh));
    if (hc.stage(L))
        return hc.rc;
    Slot &s = hc.slot();
    ebvo_edge *kfL = hc.at<ebvo_edge>(o_kfL), *kfR = hc.at<ebvo_edge>(o_kfR), *cfL = hc.at<ebvo_edge>(o_cfL), *cfR = hc.at<ebvo_edge>(o_cfR);
    double *pl = hc.at<double>(o_pl), *pr = hc.at<double>(o_pr);
    unsigned long long *d_tot = hc.at<unsigned long long>(o_tot);
    int32_t *d_rows = hc.at<int32_t>(o_rows);
    uint8_t *on = hc.at<uint8_t>(o_on);
    void *grid = hc.at<char>(o_grid);
    if (hc.fill(d_tot, 0, sizeof(unsigned long long) * 8) || hc.up(kfL, kf_left, eb * nz) || hc.up(kfR, kf_right, eb * nz) ||
        hc.up(pl, proj_left, sizeof(double) * 2 * nz) || hc.up(pr, proj_right, sizeof(double) * 2 * nz) ||
        (row_on ? hc.up(on, row_on, nz) : hc.fill(on, 1, nz)) || hc.fill(d_rows, 0, sizeof(int32_t) * 2 * nz))
        return hc.rc;
    int rc;
    if (n_kf > 0 && n_cf > 0)
    {
        if (hc.up(cfL, cf_left, eb * ncz) || hc.up(cfR, cf_right, eb * ncz))
            return hc.rc;
        if ((rc = match_temporal_cells_enqueue(ctx, s, cfL, cfR, n_cf, cell_size, gw, gh, grid)) ||
            (rc = tgt_grid_rows_enqueue(ctx, s, kfL, kfR, n_kf, cfL, cfR, grid, n_cf, cell_size, tgt_cell_radius(grid_radius, cell_size), gw, gh,
                                        on, pl, pr, tp_dist, d_rows, d_tot)))
            return rc;
    }
    else if ((rc = gt_totals_enqueue(ctx, s, d_rows, on, n_kf, d_tot))) // no current-frame mates: the rows that are on are empty
        return rc;
    return host_stage_tail(hc, d_rows, d_tot, n_kf, row_on, /*temporal=*/true, n_tp, stage_out);
}

// The middle of a two-pass call: the per-row counts of the first pass come back (d_cnt null: nothing was counted, every row
// is empty), the call's copies end, and the row offsets are formed.  EBVO_ERR_CAPACITY: more than a 32-bit offset holds.
static int host_row_offsets(HostCall &hc, const int32_t *d_cnt, int n_kf, std::vector<int32_t> &h_rp)
{
    std::vector<int32_t> h_cnt((size_t)n_kf + 1, 0);
    int32_t n_rows = 0;
    hc.down(h_cnt.data(), d_cnt, d_cnt ? sizeof(int32_t) * (size_t)n_kf : 0);
    if (hc.finish()) // on every path, before h_cnt goes
        return hc.rc;
    return tgt_row_offsets(h_cnt, n_kf, h_rp, &n_rows) ? EBVO_OK : EBVO_ERR_CAPACITY;
}

// the per-mate arrays of a two-pass call: in the image (or live), both projections, both orientations
struct MateArrays
{
    uint8_t *flag;
    double *pl, *pr, *ol, *orr;
};

// The end of a two-pass call: the per-mate outputs the caller asked for, and the wait.
static int host_mate_outputs(HostCall &hc, size_t nz, const MateArrays &host, const MateArrays &dev)
{
    hc.down(host.flag, dev.flag, nz);
    hc.down(host.pl, dev.pl, sizeof(double) * 2 * nz);
    hc.down(host.pr, dev.pr, sizeof(double) * 2 * nz);
    hc.down(host.ol, dev.ol, sizeof(double) * nz);
    hc.down(host.orr, dev.orr, sizeof(double) * nz);
    return hc.finish();
}

extern "C" int ebvo_tgt_veridical(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, const double *kf_gamma, int n_kf,
                                  const ebvo_edge *cf_left, const ebvo_edge *cf_right, int n_cf, int img_w, int img_h, int cell_size,
                                  const double R[9], const double t[3], const ebvo_stereo_calib *calib, const ebvo_tgt_params *params,
                                  uint8_t *in_image, double *proj_left, double *proj_right, double *orient_left, double *orient_right,
                                  int32_t *ver_row_ptr, int32_t *ver_idx, int64_t cap, int64_t *n_veridical)
{
    ebvo_tgt_params P;
    ebvo_tgt_default_params(&P);
    if (params)
        P = *params;
    if (!ctx || n_kf < 0 || n_cf < 0 || img_w < 1 || img_h < 1 || cell_size < 1 || cap < 0 || !tgt_pose_ok(R, t, calib) || !tgt_params_ok(&P) ||
        (n_kf > 0 && (!kf_left || !kf_right)) || (n_cf > 0 && (!cf_left || !cf_right)))
        return EBVO_ERR_ARG;
    const int64_t gw64 = ((int64_t)img_w + cell_size - 1) / cell_size, gh64 = ((int64_t)img_h + cell_size - 1) / cell_size;
    if (gw64 * gh64 > (1 << 26) || gw64 > 30000 || gh64 > 30000) // the cells of a mate are 16-bit
        return EBVO_ERR_ARG;
    std::vector<int32_t> h_rp;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    if (n_veridical)
        *n_veridical = 0;
    const int gw = (int)gw64, gh = (int)gh64;
    const size_t nz = (size_t)n_kf, ncz = (size_t)n_cf;
    // mates, gamma, the six doubles per keyframe mate, counts and offsets, flags, the grid, the list
    const size_t eb = sizeof(ebvo_edge), idx_room = sizeof(int32_t) * (size_t)((cap < (int64_t)nz * ncz ? cap : (int64_t)nz * ncz) + 1);
    Carve L;
    const size_t o_kfL = L.take(eb * nz), o_kfR = L.take(eb * nz), o_cfL = L.take(eb * ncz), o_cfR = L.take(eb * ncz),
                 o_pl = L.take(sizeof(double) * 2 * nz), o_pr = L.take(sizeof(double) * 2 * nz), o_ol = L.take(sizeof(double) * nz),
                 o_or = L.take(sizeof(double) * nz), o_gamma = L.take(sizeof(double) * 3 * nz), o_cnt = L.take(sizeof(int32_t) * (nz + 1)),
                 o_rp = L.take(sizeof(int32_t) * (nz + 1)), o_in = L.take(nz), o_on = L.take(nz),
                 o_grid = L.take(match_temporal_grid_bytes(n_cf, gw * gh)), o_idx = L.take(idx_room);
    if (hc.stage(L))
        return hc.rc;
    Slot &s = hc.slot();
    ebvo_edge *kfL = hc.at<ebvo_edge>(o_kfL), *kfR = hc.at<ebvo_edge>(o_kfR), *cfL = hc.at<ebvo_edge>(o_cfL), *cfR = hc.at<ebvo_edge>(o_cfR);
    double *pl = hc.at<double>(o_pl), *pr = hc.at<double>(o_pr), *ol = hc.at<double>(o_ol), *orr = hc.at<double>(o_or);
    double *gamma = kf_gamma ? hc.at<double>(o_gamma) : nullptr;
    int32_t *cnt = hc.at<int32_t>(o_cnt), *rp = hc.at<int32_t>(o_rp), *idx = hc.at<int32_t>(o_idx);
    uint8_t *in = hc.at<uint8_t>(o_in), *on = hc.at<uint8_t>(o_on);
    void *grid = hc.at<char>(o_grid);
    if (hc.up(kfL, kf_left, eb * nz) || hc.up(kfR, kf_right, eb * nz) || hc.up(gamma, kf_gamma, sizeof(double) * 3 * nz))
        return hc.rc;
    int rc;
    if ((rc = tgt_project_enqueue(ctx, s, kfL, kfR, gamma, n_kf, R, t, calib, P.img_margin, img_w, img_h, in, pl, pr, ol, orr)))
        return rc;
    const bool walk = n_kf > 0 && n_cf > 0;
    const int sr = tgt_cell_radius(P.search_radius, cell_size);
    if (walk)
    {
        if (hc.up(cfL, cf_left, eb * ncz) || hc.up(cfR, cf_right, eb * ncz))
            return hc.rc;
        if ((rc = match_temporal_cells_enqueue(ctx, s, cfL, cfR, n_cf, cell_size, gw, gh, grid)) ||
            (rc = tgt_veridical_enqueue(ctx, s, n_kf, in, pl, pr, ol, orr, cfL, cfR, grid, n_cf, cell_size, sr, gw, gh, P.tp_dist,
                                        P.orient_thr_deg, nullptr, cnt, nullptr, nullptr, 0, nullptr)))
            return rc;
    }
    if ((rc = host_row_offsets(hc, walk ? cnt : nullptr, n_kf, h_rp)))
        return rc;
    const int64_t n_ver = h_rp[n_kf];
    if (n_veridical)
        *n_veridical = n_ver;
    if (ver_idx && n_ver > cap)
        return EBVO_ERR_CAPACITY;
    if (walk && ver_idx && n_ver > 0)
    {
        if (hc.up(rp, h_rp.data(), sizeof(int32_t) * (nz + 1)))
            return hc.rc;
        if ((rc = tgt_veridical_enqueue(ctx, s, n_kf, in, pl, pr, ol, orr, cfL, cfR, grid, n_cf, cell_size, sr, gw, gh, P.tp_dist,
                                        P.orient_thr_deg, nullptr, nullptr, rp, idx, n_ver, on)))
            return rc;
        hc.down(ver_idx, idx, sizeof(int32_t) * (size_t)n_ver);
    }
    if (host_mate_outputs(hc, nz, {in_image, proj_left, proj_right, orient_left, orient_right}, {in, pl, pr, ol, orr}))
        return hc.rc;
    if (ver_row_ptr)
        memcpy(ver_row_ptr, h_rp.data(), sizeof(int32_t) * (nz + 1));
    return EBVO_OK;
}

// ---- temporal matching under a pose prior ---------------------------------------------------------------------------------
extern "C" void ebvo_tprior_default_params(ebvo_tprior_params *p)
{
    if (!p)
        return;
    p->img_margin = 0.0;
    p->use_orientation = 1;
}

static bool tprior_args_ok(const double *R, const double *t, const ebvo_stereo_calib *calib, const ebvo_tprior_params *P)
{
    if (!tgt_pose_ok(R, t, calib) || !(P->img_margin >= 0 && std::isfinite(P->img_margin)))
        return false;
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(R[k]))
            return false;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(t[k]))
            return false;
    return true;
}

extern "C" int ebvo_temporal_set_prior(ebvo_ctx *ctx, int slot, const double R[9], const double t[3], const ebvo_stereo_calib *calib,
                                       const ebvo_tprior_params *params)
{
    ebvo_tprior_params P;
    ebvo_tprior_default_params(&P);
    if (params)
        P = *params;
    Slot *sp;
    if (get_slot(ctx, slot, &sp) || !tprior_args_ok(R, t, calib, &P))
        return EBVO_ERR_ARG;
    if (sp->tq_in_flight)
    {
        ctx->last_error = "a temporal match is in flight in the slot (ebvo_temporal_match_wait first)";
        return EBVO_ERR_STATE;
    }
    Slot::TqPrior &N = sp->tq_prior_next; // read by the next ebvo_temporal_match_submit; the slot's match stays
    N.on = true;
    memcpy(N.R, R, sizeof N.R);
    memcpy(N.t, t, sizeof N.t);
    N.calib = *calib;
    N.P = P;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_clear_prior(ebvo_ctx *ctx, int slot)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    if (sp->tq_in_flight)
    {
        ctx->last_error = "a temporal match is in flight in the slot (ebvo_temporal_match_wait first)";
        return EBVO_ERR_STATE;
    }
    sp->tq_prior_next.on = false;
    return EBVO_OK;
}

extern "C" int ebvo_temporal_prior_fetch(ebvo_ctx *ctx, int slot, uint8_t *live, double *proj_left, double *proj_right,
                                         double *orient_left, double *orient_right)
{
    Slot *sp;
    if (get_slot(ctx, slot, &sp))
        return EBVO_ERR_ARG;
    Slot &s = *sp;
    if (s.tq_n < 0 || s.in_flight || s.tq_in_flight || !s.tq_prior.on)
    {
        ctx->last_error = s.in_flight || s.tq_in_flight ? "the slot has work in flight (wait for it first)"
                          : s.tq_n < 0                  ? "the slot holds no temporal match (ebvo_temporal_match first)"
                                                        : "the slot's match was made without a prior (ebvo_temporal_set_prior before the match)";
        return EBVO_ERR_STATE;
    }
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nz = (size_t)s.tq_n_kf;
    if (!nz)
        return EBVO_OK;
    const TemporalPrior Q = temporal_prior_view(s);
    const struct
    {
        void *dst;
        const void *src;
        size_t bytes;
    } copies[] = {{live, Q.live, nz}, {proj_left, Q.pl, sizeof(double) * 2 * nz}, {proj_right, Q.pr, sizeof(double) * 2 * nz},
                  {orient_left, Q.ol, sizeof(double) * nz}, {orient_right, Q.orr, sizeof(double) * nz}};
    for (const auto &c : copies)
        if (c.dst)
            EBVO_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s.stream));
    EBVO_HIP(ctx, hipStreamSynchronize(s.stream));
    return EBVO_OK;
}

extern "C" int ebvo_tprior_candidates(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf,
                                      const ebvo_edge *cf_left, const ebvo_edge *cf_right, int n_cf, int img_w, int img_h, int cell_size,
                                      double grid_radius, double orient_thr_deg, const double R[9], const double t[3],
                                      const ebvo_stereo_calib *calib, const ebvo_tprior_params *params, uint8_t *live, double *proj_left,
                                      double *proj_right, double *orient_left, double *orient_right, int32_t *row_ptr, int32_t *col_idx,
                                      int64_t cap, int64_t *n_candidates)
{
    ebvo_tprior_params P;
    ebvo_tprior_default_params(&P);
    if (params)
        P = *params;
    if (!ctx || n_kf < 0 || n_cf < 0 || img_w < 1 || img_h < 1 || cell_size < 1 || cap < 0 ||
        !(grid_radius >= 0 && std::isfinite(grid_radius)) || !(orient_thr_deg >= 0) || !tprior_args_ok(R, t, calib, &P) ||
        (n_kf > 0 && (!kf_left || !kf_right)) || (n_cf > 0 && (!cf_left || !cf_right)))
        return EBVO_ERR_ARG;
    const int64_t gw64 = ((int64_t)img_w + cell_size - 1) / cell_size, gh64 = ((int64_t)img_h + cell_size - 1) / cell_size;
    if (gw64 * gh64 > (1 << 26) || gw64 > 30000 || gh64 > 30000) // the cells of a mate are 16-bit
        return EBVO_ERR_ARG;
    std::vector<int32_t> h_rp;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    if (n_candidates)
        *n_candidates = 0;
    const int gw = (int)gw64, gh = (int)gh64;
    const size_t nz = (size_t)n_kf, ncz = (size_t)n_cf;
    // mates, the six doubles per keyframe mate, counts and offsets, live, the grid, the list
    const size_t eb = sizeof(ebvo_edge), idx_room = sizeof(int32_t) * (size_t)((cap < (int64_t)nz * ncz ? cap : (int64_t)nz * ncz) + 1);
    Carve L;
    const size_t o_kfL = L.take(eb * nz), o_kfR = L.take(eb * nz), o_cfL = L.take(eb * ncz), o_cfR = L.take(eb * ncz),
                 o_pl = L.take(sizeof(double) * 2 * nz), o_pr = L.take(sizeof(double) * 2 * nz), o_ol = L.take(sizeof(double) * nz),
                 o_or = L.take(sizeof(double) * nz), o_cnt = L.take(sizeof(int32_t) * (nz + 1)), o_rp = L.take(sizeof(int32_t) * (nz + 1)),
                 o_lv = L.take(nz), o_grid = L.take(match_temporal_grid_bytes(n_cf, gw * gh)), o_idx = L.take(idx_room);
    if (hc.stage(L))
        return hc.rc;
    Slot &s = hc.slot();
    ebvo_edge *kfL = hc.at<ebvo_edge>(o_kfL), *kfR = hc.at<ebvo_edge>(o_kfR), *cfL = hc.at<ebvo_edge>(o_cfL), *cfR = hc.at<ebvo_edge>(o_cfR);
    double *pl = hc.at<double>(o_pl), *pr = hc.at<double>(o_pr), *ol = hc.at<double>(o_ol), *orr = hc.at<double>(o_or);
    int32_t *cnt = hc.at<int32_t>(o_cnt), *rp = hc.at<int32_t>(o_rp), *idx = hc.at<int32_t>(o_idx);
    uint8_t *lv = hc.at<uint8_t>(o_lv);
    void *grid = hc.at<char>(o_grid);
    TemporalPrior Q;
    Q.live = lv; Q.pl = pl; Q.pr = pr; Q.ol = ol; Q.orr = orr;
    Q.use_orientation = P.use_orientation != 0;
    if (hc.fill(cnt, 0, sizeof(int32_t) * (nz + 1)) || hc.fill(rp, 0, sizeof(int32_t) * (nz + 1)) || hc.up(kfL, kf_left, eb * nz) ||
        hc.up(kfR, kf_right, eb * nz))
        return hc.rc;
    int rc;
    if ((rc = tprior_project_enqueue(ctx, s, kfL, kfR, n_kf, R, t, calib, P.img_margin, img_w, img_h, lv, pl, pr, ol, orr)))
        return rc;
    const bool walk = n_kf > 0 && n_cf > 0;
    const int sr = tgt_cell_radius(grid_radius, cell_size);
    if (walk)
    {
        if (hc.up(cfL, cf_left, eb * ncz) || hc.up(cfR, cf_right, eb * ncz))
            return hc.rc;
        if ((rc = match_temporal_cells_enqueue(ctx, s, cfL, cfR, n_cf, cell_size, gw, gh, grid)) ||
            (rc = match_temporal_candidates_enqueue(ctx, s, kfL, kfR, n_kf, cfL, cfR, grid, n_cf, cell_size, sr, gw, gh, orient_thr_deg, cnt,
                                                    nullptr, nullptr, 0, &Q)))
            return rc;
    }
    if ((rc = host_row_offsets(hc, walk ? cnt : nullptr, n_kf, h_rp)))
    {
        if (rc == EBVO_ERR_CAPACITY)
            ctx->last_error = "more candidate quads than a 32-bit row offset holds";
        return rc;
    }
    const int64_t n_cand = h_rp[n_kf];
    if (n_candidates)
        *n_candidates = n_cand;
    if (col_idx && n_cand > cap)
    {
        ctx->last_error = "ebvo_tprior_candidates: " + std::to_string(n_cand) + " candidate quads";
        return EBVO_ERR_CAPACITY;
    }
    if (walk && col_idx && n_cand > 0)
    {
        if (hc.up(rp, h_rp.data(), sizeof(int32_t) * (nz + 1)))
            return hc.rc;
        if ((rc = match_temporal_candidates_enqueue(ctx, s, kfL, kfR, n_kf, cfL, cfR, grid, n_cf, cell_size, sr, gw, gh, orient_thr_deg,
                                                    nullptr, rp, idx, n_cand, &Q)))
            return rc;
        hc.down(col_idx, idx, sizeof(int32_t) * (size_t)n_cand);
    }
    if (host_mate_outputs(hc, nz, {live, proj_left, proj_right, orient_left, orient_right}, {lv, pl, pr, ol, orr}))
        return hc.rc;
    if (row_ptr)
        memcpy(row_ptr, h_rp.data(), sizeof(int32_t) * (nz + 1));
    return EBVO_OK;
}

extern "C" int ebvo_tgt_evaluate_rows(ebvo_ctx *ctx, const int32_t *row_ptr, const ebvo_edge *left_centres, const ebvo_edge *right_centres,
                                      int n_kf, const uint8_t *row_on, const double *proj_left, const double *proj_right, double tp_dist,
                                      int32_t *n_tp, uint8_t *is_tp, ebvo_gt_stage *stage_out)
{
    int64_t np = 0;
    if (!ctx || !stage_out || !(tp_dist >= 0) || check_csr(row_ptr, n_kf, &np) || (n_kf > 0 && (!proj_left || !proj_right)) ||
        (np > 0 && (!left_centres || !right_centres)))
        return EBVO_ERR_ARG;
    HostCall hc(ctx);
    if (hc.rc)
        return hc.rc;
    memset(stage_out, 0, sizeof *stage_out);
    stage_out->present = 1;
    const size_t nz = (size_t)n_kf, npz = (size_t)np;
    // both centre lists, both projections, the totals, the (n, tp) rows, row_ptr, row_on, is_tp
    Carve L;
    const size_t o_cL = L.take(sizeof(ebvo_edge) * (npz + 1)), o_cR = L.take(sizeof(ebvo_edge) * (npz + 1)),
                 o_pl = L.take(sizeof(double) * 2 * (nz + 1)), o_pr = L.take(sizeof(double) * 2 * (nz + 1)),
                 o_tot = L.take(sizeof(unsigned long long) * 8), o_rows = L.take(sizeof(int32_t) * 2 * (nz + 1)),
                 o_rp = L.take(sizeof(int32_t) * (nz + 2)), o_on = L.take(nz), o_tp = L.take(npz);
    if (hc.stage(L))
        return hc.rc;
    ebvo_edge *cL = hc.at<ebvo_edge>(o_cL), *cR = hc.at<ebvo_edge>(o_cR);
    double *pl = hc.at<double>(o_pl), *pr = hc.at<double>(o_pr);
    unsigned long long *d_tot = hc.at<unsigned long long>(o_tot);
    int32_t *d_rows = hc.at<int32_t>(o_rows), *d_rp = hc.at<int32_t>(o_rp);
    uint8_t *on = hc.at<uint8_t>(o_on), *d_tp = hc.at<uint8_t>(o_tp);
    if (hc.up(cL, left_centres, sizeof(ebvo_edge) * npz) || hc.up(cR, right_centres, sizeof(ebvo_edge) * npz) ||
        hc.up(d_rp, row_ptr, sizeof(int32_t) * (nz + 1)) || hc.up(pl, proj_left, sizeof(double) * 2 * nz) ||
        hc.up(pr, proj_right, sizeof(double) * 2 * nz) || (row_on ? hc.up(on, row_on, nz) : hc.fill(on, 1, nz)) ||
        hc.fill(d_rows, 0, sizeof(int32_t) * 2 * nz))
        return hc.rc;
    if (int rc = tgt_rows_enqueue(ctx, hc.slot(), d_rp, cL, cR, nullptr, nullptr, nullptr, nullptr, pl, pr, on, n_kf, np, tp_dist, d_rows, d_tp,
                                  d_tot))
        return rc;
    hc.down(is_tp, d_tp, npz);
    return host_stage_tail(hc, d_rows, d_tot, n_kf, row_on, /*temporal=*/true, n_tp, stage_out);
}

// the values each developer key accepts; anything else is refused before the context changes at all
static bool debug_value_ok(int key, int value)
{
    switch (key)
    {
    case 4: case 7: case 10: case 13: case 14:
        return value <= 1;
    case 8:
        return value == 2 || value == 3;
    case 6:
        return value >= 1;
    case 11: case 12:
        return value <= EBVO_DEBUG_MAX_EXACT_BLOCKS;
    case 9:
        return value <= EBVO_DEBUG_MAX_GN_BLOCKS;
    case 18:
        return value <= 512; // the smallest of the grids it divides: a larger divisor would launch zero blocks
    case 19:
        return value <= EBVO_TOTAL_PARTS;
    case 20:
        return value <= 1 << 20;
    case 21:
        return value <= EBVO_DEBUG_MAX_GT_BLOCKS;
    case 22:
        return value <= EBVO_DEBUG_MAX_TEMPORAL_BLOCKS;
    case EBVO_DEBUG_KEY_FINALIZE_BLOCKS:
        return value <= EBVO_DEBUG_MAX_FINALIZE_BLOCKS;
    case 0: case 1: case 2: case 3: case 5: case 15: case 16: case 17:
        return true;
    default:
        return false;
    }
}

extern "C" int ebvo_debug_set(ebvo_ctx *ctx, int key, int value)
{
    if (!ctx || value < 0 || !debug_value_ok(key, value))
        return EBVO_ERR_ARG;
    ++ctx->graph_gen;
    if (key == 10)
        ctx->use_graphs = value; // the pair chain as a hipGraph (default) or as direct launches
    else if (key == 14)
        ctx->no_prep = value;
    else if (key == 11 || key == 12)
        ctx->exact_blocks[key - 11] = value;
    else if (key == 15)
        ctx->repeat_mask = value;
    else if (key == 16)
        ctx->stop_stage = value;
    else if (key == 17)
        ctx->ncc_blocks = value;
    else if (key == 18)
        ctx->small_div = value;
    else if (key == 19)
        ctx->cand_blocks = value;
    else if (key == 20)
        ctx->pose_batch = value; // draws per batch of the pose search (same bits for any value)
    else if (key == 21)
        ctx->gt_blocks = value; // grid of the ground-truth kernels (same bits for any value)
    else if (key == 22)
        ctx->temporal_blocks = value; // cap on the temporal path's grids (same bits for any value)
    else if (key == EBVO_DEBUG_KEY_FINALIZE_BLOCKS)
        ctx->finalize_blocks = value; // cap on the stereo finalize chain's grids (same bits for any value)
    else if (key == 13)
        ctx->ingest_stream = value;
    else if (key == 0)
        ctx->wait_attempts = value;
    else if (key == 1)
        ctx->force_overflow = value;
    else if (key == 2)
        ctx->lanes = value; // 0 = one stream per slot whatever their number
    else if (key == 3)
        ctx->prof_only = value - 1; // 0 = every stage; id + 1 = that stage alone: no event markers between the other kernels
    else if (key == 4)
        ctx->gn_no_rows = value; // refinement launch layout (same bits either way, tests/test_gpu_refine.py)
    else if (key == 5)
        ctx->gn_rows_below = value;
    else if (key == 9)
        ctx->gn_persist_blocks = value;
    else if (key == 8)
        ctx->gn_persist_waves = value;
    else if (key == 7)
        ctx->gn_per_iteration_rows = value; // the stereo refinement's row layout as a launch per iteration (A/B and parity tests)
    else // key 6
    {
        for (Slot *sl : ctx->slots) // test hook: the next temporal match of every slot finds its quad buffers too small
            if (sl->tq_cap > 0 && !sl->tq_in_flight)
                sl->tq_cap = value;
    }
    return EBVO_OK;
}

extern "C" int ebvo_fp64_peak(ebvo_ctx *ctx, int iters, double *tflops_muladd, double *tflops_fma)
{
    if (!ctx || iters <= 0)
        return EBVO_ERR_ARG;
    EBVO_HIP(ctx, hipSetDevice(ctx->device));
    return misc_fp64_peak(ctx, *ctx->slots[0], iters, tflops_muladd, tflops_fma);
}
