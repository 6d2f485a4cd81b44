// C ABI of libscarplet_hip.so (include/scarplet_hip.h): context, DEM hand-over,
// batching of templates into orientation runs, and measurement hooks.
#include "sc_internal.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <math.h>
#include <algorithm>

// ---------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------
int sc_fail(sc_ctx* ctx, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

// hipMalloc for the context's buffers and the template cache's entries.  TEST HOOK "test_mem_gb" > 0 (not a public
// option: tests/test_gpu_templ_cache.py alone sets it): out of memory is answered where the two together would pass
// that bound, so that the allocation-pressure path below runs on a device that has room to spare.
static hipError_t sc_device_alloc(sc_ctx* ctx, void** p, size_t bytes) {
    if (ctx->test_mem_gb > 0.0 && (double)sc_total_bytes(ctx) + (double)ctx->tc.held + (double)bytes > ctx->test_mem_gb * 1e9)
        return hipErrorOutOfMemory;
    return hipMalloc(p, bytes);
}

int sc_ensure(sc_ctx* ctx, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap && b.p) return SC_OK;
    if (b.p) {
        SC_HIP(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    if (bytes == 0) bytes = 16;
    // no allocation of the context fails for the template cache: its entries go, least recently used first, before
    // out-of-memory is reported (all but the chunk's whose launches are being put together: ctx->tc_cur)
    hipError_t e = sc_device_alloc(ctx, &b.p, bytes);
    while (e == hipErrorOutOfMemory && ctx->tc.drop_lru(ctx->tc_cur, true)) {
        (void)hipGetLastError();
        e = sc_device_alloc(ctx, &b.p, bytes);
    }
    if (e != hipSuccess) b.p = nullptr;
    SC_HIP(ctx, e);
    b.cap = bytes;
    return SC_OK;
}

// ---------------------------------------------------------------------------
// template coefficient planes kept across searches (sc_templ_cache.h holds key, budget and LRU)
// ---------------------------------------------------------------------------
static void* templ_cache_alloc(void* user, size_t bytes) {
    void* p = nullptr;
    if (sc_device_alloc((sc_ctx*)user, &p, bytes) != hipSuccess) {
        (void)hipGetLastError();             // (no memory: the chunk runs uncached, the search does not fail)
        return nullptr;
    }
    return p;
}
static void templ_cache_free(void* user, void* mem) {
    sc_ctx* ctx = (sc_ctx*)user;
    (void)hipStreamSynchronize(ctx->stream);     // (launches of the search in flight may still read the entry)
    (void)hipFree(mem);
}

// What k_windows adds up on the device (count(W != 0) and sum(W**2) in sums, sum|W| in wl1) travels with the planes:
// src -> dst for n templates, from the search's tables into the entry on a miss and back on a hit.
__global__ void __launch_bounds__(64)
k_templ_sums(const double* __restrict__ src_sums, const double* __restrict__ src_wl1, double* __restrict__ dst_sums,
             double* __restrict__ dst_wl1, int n) {
    for (int i = blockIdx.x * 64 + threadIdx.x; i < 3 * n; i += gridDim.x * 64) {
        if (i < 2 * n) dst_sums[i] = src_sums[i];
        else dst_wl1[i - 2 * n] = src_wl1[i - 2 * n];
    }
}

// The budget of a search, once fft_prepare has its buffers: option "templ_gb" in GB (0: off), or - automatic - half of
// what is free on the device, the entries already held counted as free.  The automatic budget is worked out at the
// search's first miss (templ_cache_entry): a search served from the cache alone asks the driver nothing.
static void templ_cache_budget(sc_ctx* ctx) {
    ctx->tc_budget_due = ctx->templ_gb < 0.0;
    if (!ctx->tc_budget_due) ctx->tc.set_budget((size_t)(ctx->templ_gb * 1e9));
    ctx->tc.begin_search();
}
static void templ_cache_budget_auto(sc_ctx* ctx) {
    size_t free_b = 0, total_b = 0;
    const double budget = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? 0.5 * ((double)free_b + (double)ctx->tc.held) : 0.0;
    ctx->tc.set_budget((size_t)budget);
    ctx->tc_budget_due = false;
}

// The entry of chunk c, if it is one the cache takes: symmetric built-in templates on an FFT route that leaves real
// coefficient planes (generic templates - complex spectra in vh - and caller-owned windows keep the uncached path).
// *hit: the entry holds the planes; else it is new and the chain fills it.  nullptr: uncached.
static TemplEntry* templ_cache_entry(sc_ctx* ctx, const sc_template* t, const MatchChunk& c, const FftGeom& fg, bool* hit) {
    *hit = false;
    if (ctx->templ_gb == 0.0 || c.parity == 0) return nullptr;
    const FftTemplFwd how = fft_route(fft_route_in(ctx, fg, c.parity)).templ;
    if (how != FFT_TEMPL_COLS_SYM && how != FFT_TEMPL_SPLIT_SYM) return nullptr;
    const int n_all = c.nb * c.n;
    const Geom& g = ctx->g;
    int pmin = INT_MAX, pmax = INT_MIN, qmin = INT_MAX, qmax = INT_MIN;
    for (int j = c.first; j < c.first + n_all; ++j) {
        if (t[j].kind != SC_KIND_SCARP && t[j].kind != SC_KIND_RICKER) return nullptr;
        pmin = std::min(pmin, t[j].pmin); pmax = std::max(pmax, t[j].pmax);
        qmin = std::min(qmin, t[j].qmin); qmax = std::max(qmax, t[j].qmax);
    }
    // (check_templates: the boxes lie on the grid)
    if ((int)ctx->h_yaxis.size() != g.ny || (int)ctx->h_xaxis.size() != g.nx) return nullptr;
    TemplKeyIn in{};
    in.t = t + c.first; in.nb = c.nb; in.n = c.n;
    in.dx = ctx->dx; in.dy = ctx->dy; in.oy = g.oy; in.ox = g.ox;
    in.Ty = fg.Ty; in.Tx = fg.Tx; in.route = (int)how; in.parity = c.parity;
    in.build_id = sc_build_id();
    in.xs = ctx->h_xaxis.data() + g.nx / 2 + qmin; in.nxs = qmax - qmin + 1;
    in.ys = ctx->h_yaxis.data() + g.ny / 2 + pmin; in.nys = pmax - pmin + 1;
    const TemplKey key = sc_templ_key(in);
    if (TemplEntry* e = ctx->tc.find(key)) {
        *hit = true;
        return e;
    }
    if (ctx->tc_budget_due) templ_cache_budget_auto(ctx);
    const size_t planes = 2 * fft_templ_plane_bytes(fg.Ty, fg.Tx) * (size_t)n_all;
    return ctx->tc.insert(key, planes + 3 * sizeof(double) * (size_t)n_all, c.nb);
}

// an entry's planes and sums as the current chunk's (e == nullptr: the context's own buffers)
static void templ_cache_use(sc_ctx* ctx, const TemplEntry* e, const FftGeom& fg, int n_all) {
    ctx->tc_cur = e;
    ctx->tc_wh = ctx->tc_mh = nullptr;
    if (!e) return;
    ctx->tc_wh = e->mem;
    ctx->tc_mh = (char*)e->mem + fft_templ_plane_bytes(fg.Ty, fg.Tx) * (size_t)n_all;
}
// sums / wl1 of templates [first, first + n_all) between the search's tables and the entry (save: into the entry)
static int templ_cache_sums(sc_ctx* ctx, const TemplEntry* e, const FftGeom& fg, int first, int n_all, bool save) {
    double* e_sums = (double*)((char*)e->mem + 2 * fft_templ_plane_bytes(fg.Ty, fg.Tx) * (size_t)n_all);
    double* e_wl1 = e_sums + 2 * (size_t)n_all;
    double* c_sums = (double*)ctx->sums.p + 2 * (size_t)first;
    double* c_wl1 = (double*)ctx->wl1.p + first;
    const unsigned blocks = (unsigned)std::min(64, (3 * n_all + 63) / 64);
    if (save)
        hipLaunchKernelGGL(k_templ_sums, dim3(blocks), dim3(64), 0, ctx->stream, c_sums, c_wl1, e_sums, e_wl1, n_all);
    else
        hipLaunchKernelGGL(k_templ_sums, dim3(blocks), dim3(64), 0, ctx->stream, e_sums, e_wl1, c_sums, c_wl1, n_all);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static void buf_free(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

size_t sc_total_bytes(sc_ctx* c) {
    DevBuf* arr[] = {&c->z, &c->xaxis, &c->yaxis, &c->A, &c->B, &c->C, &c->curv,
                     &c->best_snr, &c->best_amp, &c->best_id, &c->map_amp,
                     &c->map_snr, &c->templ, &c->sums, &c->wl1, &c->norms, &c->norm_part, &c->win_w, &c->win_m,
                     &c->tw_y, &c->tw_x, &c->blk, &c->cblk, &c->uc, &c->uc2, &c->vh, &c->wh, &c->mh,
                     &c->yw, &c->ym, &c->tiles, &c->halo_z, &c->halo_stage, &c->res, &c->sib_buf, &c->dwin, &c->spans, &c->res_stats, &c->digest, &c->split_s, &c->split_a, &c->split_i,
                     &c->near, &c->near_ev, &c->score, &c->score_w, &c->score_abc, &c->st_slot, &c->st_work, &c->st_pairs, &c->st_patch, &c->st_spans, &c->snap, &c->xch, &c->xch_cnt,
                     &c->tr_planes, &c->tr_thin, &c->tr_par, &c->tr_lab, &c->tr_cnt, &c->tr_bsum, &c->tr_tot, &c->tr_sort, &c->tr_hist, &c->tr_rbsum, &c->tr_seg,
                     &c->pf_z, &c->pf_cells, &c->pf_dir, &c->pf_ages, &c->pf_tab, &c->pf_rows, &c->pf_sse, &c->pf_shift, &c->pf_wt, &c->pf_ftab, &c->pf_terms,
                     &c->sg_z, &c->sg_ages, &c->sg_tab, &c->sg_cells, &c->sg_dir, &c->sg_cseg, &c->sg_start, &c->sg_blk, &c->sg_label, &c->sg_prof, &c->sg_int,
                     &c->sg_scal, &c->sg_age, &c->sg_list, &c->sg_part, &c->sg_tot, &c->sg_tsse, &c->sg_cnt, &c->sg_rows, &c->sg_out, &c->sg_sse, &c->sg_shift, &c->sg_ftab, &c->sg_width, &c->sg_fine, &c->sq_wt, &c->sq_state, &c->sq_hist, &c->sq_a,
                     &c->bs_blk, &c->bs_sblk, &c->bs_terms, &c->bs_index, &c->bs_a, &c->bs_hist, &c->bs_rows, &c->cb_rows, &c->cb_mb,
                     &c->st_win, &c->st_wstart, &c->st_spp, &c->st_rows, &c->st_sse, &c->cw_shift,
                     &c->sb_win, &c->sb_wstart, &c->sb_wblk, &c->sb_bhi, &c->sb_rows, &c->sb_hist,
                     &c->sf_work, &c->sf_cells, &c->sf_cube, &c->sf_rows};
    size_t s = 0;
    for (DevBuf* b : arr) s += b->cap;
    for (auto& w : c->windows) s += (size_t)w.h * w.wd * 13;
    return s;
}

int sc_lds_attr(sc_ctx* ctx, const void* kernel, size_t bytes) {
    auto it = ctx->lds_attr.find(kernel);
    if (it != ctx->lds_attr.end() && it->second >= bytes) return SC_OK;
    SC_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)bytes));
    ctx->lds_attr[kernel] = bytes;
    return SC_OK;
}

// ---------------------------------------------------------------------------
// profiling: HIP events on the context's stream around sampled launches
// ---------------------------------------------------------------------------
// A bracket may hold several launches of the same kernel (sc_prof_end's n):
// launches are counted one by one, and a sampled bracket contributes its
// elapsed time divided over its n launches.
void sc_prof_begin(sc_ctx* ctx, int kernel) {
    ctx->prof_cur = -1;
    ctx->prof_kernel = kernel;
    const long long b = ctx->k_brackets[kernel]++;
    if (!ctx->prof) return;
    // one bracket in `prof`, chosen by a hash of the counter: the launches of a
    // kernel come in periodic patterns (curvature / template forward passes, first
    // / second chunk of an orientation) that a fixed stride would alias with
    uint32_t h = (uint32_t)b * 2654435761u;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    if (ctx->prof > 1 && h % (uint32_t)ctx->prof) return;
    std::pair<hipEvent_t, hipEvent_t> ev;
    if (!ctx->ev_pool.empty()) {
        ev = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
    } else {
        if (hipEventCreate(&ev.first) != hipSuccess) return;
        if (hipEventCreate(&ev.second) != hipSuccess) return;
    }
    (void)hipEventRecord(ev.first, ctx->stream);
    ctx->prof_cur = kernel;
    ctx->prof_ev0 = ev.first;
    ctx->prof_ev1 = ev.second;
}

void sc_prof_end(sc_ctx* ctx, int n) {
    ctx->k_launches[ctx->prof_kernel] += n;
    if (ctx->prof_cur < 0) return;
    (void)hipEventRecord(ctx->prof_ev1, ctx->stream);
    ctx->pending.push_back({ctx->prof_cur, {ctx->prof_ev0, ctx->prof_ev1}});
    ctx->pending_n.push_back(n);
    ctx->prof_cur = -1;
}

void sc_prof_collect(sc_ctx* ctx) {
    for (size_t i = 0; i < ctx->pending.size(); ++i) {
        auto& p = ctx->pending[i];
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.second.first, p.second.second) == hipSuccess) {
            ctx->k_ms[p.first] += ms;
            ctx->k_sampled[p.first] += ctx->pending_n[i];
        }
        ctx->ev_pool.push_back(p.second);
    }
    ctx->pending.clear();
    ctx->pending_n.clear();
}

// ---------------------------------------------------------------------------
// lifetime
// ---------------------------------------------------------------------------
extern "C" int sc_abi_version(void) { return SC_ABI_VERSION; }

extern "C" int sc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int sc_create(int device, sc_ctx** out) {
    if (!out) return SC_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SC_ERR_HIP;
    if (device < 0 || device >= n) return SC_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return SC_ERR_HIP;
    sc_ctx* c = new sc_ctx();
    c->device = device;
    c->tc.alloc = templ_cache_alloc;
    c->tc.release = templ_cache_free;
    c->tc.user = c;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return SC_ERR_HIP;
    }
    *out = c;
    return SC_OK;
}

extern "C" int sc_set_option(sc_ctx* ctx, const char* name, double value) {
    if (!ctx || !name) return SC_ERR_INVALID;
    if (!strcmp(name, "kappa")) {
        if (!(value >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "kappa must be >= 0");
        ctx->kappa = (float)value;
    } else if (!strcmp(name, "variant")) {
        ctx->variant = (int)value;
    } else if (!strcmp(name, "batch")) {
        ctx->batch_off = value == 0.0;
    } else if (!strcmp(name, "batch_fill")) {
        if (!(value >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "batch_fill must be >= 0");
        ctx->batch_fill = (int)value;
    } else if (!strcmp(name, "i1_pairs")) {
        if (!(value >= 1.0 && value <= 64.0)) return sc_fail(ctx, SC_ERR_INVALID, "i1_pairs must be 1 .. 64");
        ctx->i1_pairs = (int)value;
    } else if (!strcmp(name, "near_window")) {
        if (!(value >= 0.0 && value < 1.0)) return sc_fail(ctx, SC_ERR_INVALID, "near_window must be in [0, 1)");
        ctx->near_w = (float)value;
    } else if (!strcmp(name, "batch_templ")) {
        if (!(value >= 0.0 && value <= (double)SC_MAX_BATCH)) return sc_fail(ctx, SC_ERR_INVALID, "batch_templ must be 0 .. %d", SC_MAX_BATCH);
        ctx->batch_templ = (int)value;
    } else if (!strcmp(name, "split_i1")) {
        if (!(value >= 0.0 && value <= 64.0)) return sc_fail(ctx, SC_ERR_INVALID, "split_i1 must be 0 .. 64");
        ctx->split_i1 = (int)value;
    } else if (!strcmp(name, "split_fill")) {
        if (!(value >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "split_fill must be >= 0");
        ctx->split_fill = (long long)value;
    } else if (!strcmp(name, "sib")) {
        ctx->sib = (int)value;
    } else if (!strcmp(name, "spectra_mb")) {
        if (!(value >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "spectra_mb must be >= 0");
        ctx->spec_mb = value;
        fft_spectra_forget(ctx);
    } else if (!strcmp(name, "fuse_fwd")) {
        ctx->fuse_fwd = value != 0.0;
    } else if (!strcmp(name, "y_gb")) {
        if (!(value >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "y_gb must be >= 0");
        ctx->y_gb = value;
    } else if (!strcmp(name, "templ_gb")) {
        if (!std::isfinite(value)) return sc_fail(ctx, SC_ERR_INVALID, "templ_gb must be finite");
        ctx->templ_gb = value < 0.0 ? -1.0 : value;          // (< 0: the automatic budget; 0: off - the entries go now)
        if (value == 0.0) {
            SC_HIP(ctx, hipSetDevice(ctx->device));
            ctx->tc.set_budget(0);
        }
    } else if (!strcmp(name, "test_mem_gb")) {            // (a test hook, not in the header's list: sc_device_alloc)
        if (!(value >= 0.0 && std::isfinite(value))) return sc_fail(ctx, SC_ERR_INVALID, "test_mem_gb must be >= 0 and finite");
        ctx->test_mem_gb = value;
    } else if (!strcmp(name, "fit_chunk")) {
        if (!(value >= 0.0 && std::isfinite(value))) return sc_fail(ctx, SC_ERR_INVALID, "fit_chunk must be >= 0 and finite");
        ctx->fit_chunk = value >= 0x1p62 ? (1ll << 62) : (long long)value;       // (it only ever lowers a built-in bound)
    } else if (!strcmp(name, "channel_terms")) {
        if (!(value == 0.0 || value == 1.0)) return sc_fail(ctx, SC_ERR_INVALID, "channel_terms must be 0 or 1");
        ctx->channel_terms = (int)value;
    } else {
        return sc_fail(ctx, SC_ERR_INVALID, "unknown option '%s'", name);
    }
    return SC_OK;
}

extern "C" int sc_clear_windows(sc_ctx* ctx) {
    if (!ctx) return SC_ERR_INVALID;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& w : ctx->windows) {
        if (!w.pooled) {
            if (w.w) (void)hipFree(w.w);
            if (w.w64) (void)hipFree(w.w64);
            if (w.m) (void)hipFree(w.m);
        }
        if (w.mask_lim) (void)hipFree(w.mask_lim);
        if (w.mask_err) (void)hipFree(w.mask_err);
    }
    ctx->windows.clear();
    for (void* p : ctx->window_pools) (void)hipFree(p);
    ctx->window_pools.clear();
    return SC_OK;
}

extern "C" void sc_destroy(sc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    sc_comm_destroy(c);
    sc_prof_collect(c);
    for (auto& e : c->ev_pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    sc_clear_windows(c);
    c->tc.clear();
    DevBuf* arr[] = {&c->z, &c->xaxis, &c->yaxis, &c->A, &c->B, &c->C, &c->curv,
                     &c->best_snr, &c->best_amp, &c->best_id, &c->map_amp,
                     &c->map_snr, &c->templ, &c->sums, &c->wl1, &c->norms, &c->norm_part, &c->win_w, &c->win_m,
                     &c->tw_y, &c->tw_x, &c->blk, &c->cblk, &c->uc, &c->uc2, &c->vh, &c->wh, &c->mh,
                     &c->yw, &c->ym, &c->tiles, &c->halo_z, &c->halo_stage, &c->res, &c->sib_buf, &c->dwin, &c->spans, &c->res_stats, &c->digest, &c->split_s, &c->split_a, &c->split_i,
                     &c->near, &c->near_ev, &c->score, &c->score_w, &c->score_abc, &c->st_slot, &c->st_work, &c->st_pairs, &c->st_patch, &c->st_spans, &c->snap, &c->xch, &c->xch_cnt,
                     &c->tr_planes, &c->tr_thin, &c->tr_par, &c->tr_lab, &c->tr_cnt, &c->tr_bsum, &c->tr_tot, &c->tr_sort, &c->tr_hist, &c->tr_rbsum, &c->tr_seg,
                     &c->pf_z, &c->pf_cells, &c->pf_dir, &c->pf_ages, &c->pf_tab, &c->pf_rows, &c->pf_sse, &c->pf_shift, &c->pf_wt, &c->pf_ftab, &c->pf_terms,
                     &c->sg_z, &c->sg_ages, &c->sg_tab, &c->sg_cells, &c->sg_dir, &c->sg_cseg, &c->sg_start, &c->sg_blk, &c->sg_label, &c->sg_prof, &c->sg_int,
                     &c->sg_scal, &c->sg_age, &c->sg_list, &c->sg_part, &c->sg_tot, &c->sg_tsse, &c->sg_cnt, &c->sg_rows, &c->sg_out, &c->sg_sse, &c->sg_shift, &c->sg_ftab, &c->sg_width, &c->sg_fine, &c->sq_wt, &c->sq_state, &c->sq_hist, &c->sq_a,
                     &c->bs_blk, &c->bs_sblk, &c->bs_terms, &c->bs_index, &c->bs_a, &c->bs_hist, &c->bs_rows, &c->cb_rows, &c->cb_mb,
                     &c->st_win, &c->st_wstart, &c->st_spp, &c->st_rows, &c->st_sse, &c->cw_shift,
                     &c->sb_win, &c->sb_wstart, &c->sb_wblk, &c->sb_bhi, &c->sb_rows, &c->sb_hist,
                     &c->sf_work, &c->sf_cells, &c->sf_cube, &c->sf_rows};
    for (DevBuf* b : arr) buf_free(*b);
    for (int k = 0; k < 4; ++k) buf_free(c->cmp[k]);
    for (int k = 0; k < 4; ++k) buf_free(c->cmp_in[k]);
    for (int k = 0; k < 4; ++k) buf_free(c->fill[k]);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" const char* sc_last_error(sc_ctx* ctx) {
    return ctx ? ctx->err.c_str() : "null context";
}

extern "C" size_t sc_device_bytes(sc_ctx* ctx) { return ctx ? sc_total_bytes(ctx) : 0; }

// ---------------------------------------------------------------------------
// DEM hand-over
// ---------------------------------------------------------------------------
static int set_dem_body(sc_ctx* ctx, int ly, int lx, int gy0, int gx0, int ny,
                        int nx, int cy0, int cy1, int cx0, int cx1, double dx,
                        double dy, int wrap, const double* xaxis,
                        const double* yaxis);

// A hand-over that fails part-way (an allocation, the digest, the curvature planes, the record's reset) leaves
// NO DEM behind: the elevations and the geometry of the old one are overwritten by then, and a context that kept
// have_dem and the new block's fingerprint would answer the same block handed over again with "unchanged" and
// search on curvature planes and kept spectra of a half-installed state.
static int set_dem_common(sc_ctx* ctx, int ly, int lx, int gy0, int gx0, int ny,
                          int nx, int cy0, int cy1, int cx0, int cx1, double dx,
                          double dy, int wrap, const double* xaxis,
                          const double* yaxis) {
    const int rc = set_dem_body(ctx, ly, lx, gy0, gx0, ny, nx, cy0, cy1, cx0, cx1, dx, dy, wrap, xaxis, yaxis);
    if (rc != SC_OK) {
        ctx->have_dem = false;
        ctx->dem_unchanged = false;
        ctx->dem_hash[0] = ctx->dem_hash[1] = 0;
        memset(ctx->dem_sig, 0, sizeof(ctx->dem_sig));
        fft_spectra_forget(ctx);
    }
    return rc;
}

static int set_dem_body(sc_ctx* ctx, int ly, int lx, int gy0, int gx0, int ny,
                        int nx, int cy0, int cy1, int cx0, int cx1, double dx,
                        double dy, int wrap, const double* xaxis,
                        const double* yaxis) {
    if (ly < 3 || lx < 3 || ny < 3 || nx < 3 || !xaxis || !yaxis)
        return sc_fail(ctx, SC_ERR_INVALID, "sc_set_dem: bad sizes or null axes");
    if (cy0 < 0 || cy1 > ny || cx0 < 0 || cx1 > nx || cy0 >= cy1 || cx0 >= cx1)
        return sc_fail(ctx, SC_ERR_INVALID, "sc_set_dem: bad core rectangle");
    if (wrap && (ly != ny || lx != nx || gy0 != 0 || gx0 != 0))
        return sc_fail(ctx, SC_ERR_INVALID, "sc_set_dem: wrap needs the whole DEM");
    if (!wrap && (cy0 < gy0 || cy1 > gy0 + ly || cx0 < gx0 || cx1 > gx0 + lx))
        return sc_fail(ctx, SC_ERR_INVALID, "sc_set_dem: core outside the block");
    if (dx == 0.0 || dy == 0.0)
        return sc_fail(ctx, SC_ERR_INVALID, "sc_set_dem: zero cell size");
    Geom& g = ctx->g;
    g.ly = ly; g.lx = lx; g.gy0 = gy0; g.gx0 = gx0; g.ny = ny; g.nx = nx;
    g.cy0 = cy0; g.cy1 = cy1; g.cx0 = cx0; g.cx1 = cx1; g.wrap = wrap ? 1 : 0;
    g.oy = ny % 2; g.ox = nx % 2;
    ctx->dx = dx; ctx->dy = dy;
    ctx->h_xaxis.assign(xaxis, xaxis + nx);
    ctx->h_yaxis.assign(yaxis, yaxis + ny);
    size_t nl = (size_t)ly * lx, nc = (size_t)(cy1 - cy0) * (cx1 - cx0);
    int rc;
    if ((rc = sc_ensure(ctx, ctx->xaxis, sizeof(double) * nx))) return rc;
    if ((rc = sc_ensure(ctx, ctx->yaxis, sizeof(double) * ny))) return rc;
    if ((rc = sc_ensure(ctx, ctx->A, sizeof(float) * nl))) return rc;
    if ((rc = sc_ensure(ctx, ctx->B, sizeof(float) * nl))) return rc;
    if ((rc = sc_ensure(ctx, ctx->C, sizeof(float) * nl))) return rc;
    if ((rc = sc_ensure(ctx, ctx->curv, sizeof(float) * nl))) return rc;
    if ((rc = sc_ensure(ctx, ctx->best_snr, sizeof(float) * nc))) return rc;
    if ((rc = sc_ensure(ctx, ctx->best_amp, sizeof(float) * nc))) return rc;
    if ((rc = sc_ensure(ctx, ctx->best_id, sizeof(uint32_t) * nc))) return rc;
    SC_HIP(ctx, hipMemcpyAsync(ctx->xaxis.p, xaxis, sizeof(double) * nx,
                               hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(ctx->yaxis.p, yaxis, sizeof(double) * ny,
                               hipMemcpyHostToDevice, ctx->stream));
    // the block's digest; a block equal to the one this context already holds - same geometry, same cell
    // size, same bits: the next sl.match of a multi-scale job on the same data (the reference runs one
    // call per scale, docs/source/examples/channels.ipynb) - keeps its curvature planes and the
    // curvature spectra kept from the last search (option "spectra_mb")
    if ((rc = sc_ensure(ctx, ctx->digest, 3 * sizeof(unsigned long long)))) return rc;
    if ((rc = launch_dem_digest(ctx, (unsigned long long*)ctx->digest.p))) return rc;
    unsigned long long dg[3] = {0, 0, 0};
    SC_HIP(ctx, hipMemcpyAsync(dg, ctx->digest.p, sizeof(dg), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double sig[16] = {(double)ly, (double)lx, (double)gy0, (double)gx0, (double)ny, (double)nx, (double)cy0,
                            (double)cy1, (double)cx0, (double)cx1, dx, dy, (double)(wrap ? 1 : 0), 0, 0, 0};
    ctx->dem_unchanged = ctx->have_dem && dg[2] == 0 && dg[0] == ctx->dem_hash[0] && dg[1] == ctx->dem_hash[1] &&
                         memcmp(sig, ctx->dem_sig, sizeof(sig)) == 0;
    ctx->dem_hash[0] = dg[0];
    ctx->dem_hash[1] = dg[1];
    ctx->dem_nan = (long long)dg[2];
    memcpy(ctx->dem_sig, sig, sizeof(sig));
    if (!ctx->dem_unchanged) {
        if ((rc = launch_curv_planes(ctx))) return rc;
        fft_spectra_forget(ctx);
    }
    ctx->have_dem = true;
    if ((rc = sc_reset_best(ctx))) return rc;
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SC_OK;
}

extern "C" int sc_dem_info(sc_ctx* ctx, long long* nan_cells, unsigned long long* hash2, int* unchanged) {
    if (!ctx) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    if (nan_cells) *nan_cells = ctx->dem_nan;
    if (hash2) { hash2[0] = ctx->dem_hash[0]; hash2[1] = ctx->dem_hash[1]; }
    if (unchanged) *unchanged = ctx->dem_unchanged ? 1 : 0;
    return SC_OK;
}

extern "C" int sc_set_dem(sc_ctx* ctx, const double* z, int ly, int lx, int gy0,
                          int gx0, int ny, int nx, int cy0, int cy1, int cx0,
                          int cx1, double dx, double dy, int wrap,
                          const double* xaxis, const double* yaxis) {
    if (!ctx || !z) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (ly < 3 || lx < 3) return sc_fail(ctx, SC_ERR_INVALID, "sc_set_dem: block too small");
    int rc = sc_ensure(ctx, ctx->z, sizeof(double) * (size_t)ly * lx);
    if (rc) return rc;
    SC_HIP(ctx, hipMemcpyAsync(ctx->z.p, z, sizeof(double) * (size_t)ly * lx,
                               hipMemcpyHostToDevice, ctx->stream));
    ctx->z_dev = (const double*)ctx->z.p;
    return set_dem_common(ctx, ly, lx, gy0, gx0, ny, nx, cy0, cy1, cx0, cx1, dx,
                          dy, wrap, xaxis, yaxis);
}

extern "C" int sc_set_dem_device(sc_ctx* ctx, const void* z_dev, int ly, int lx,
                                 int gy0, int gx0, int ny, int nx, int cy0,
                                 int cy1, int cx0, int cx1, double dx, double dy,
                                 int wrap, const double* xaxis,
                                 const double* yaxis) {
    if (!ctx || !z_dev) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    ctx->z_dev = (const double*)z_dev;
    return set_dem_common(ctx, ly, lx, gy0, gx0, ny, nx, cy0, cy1, cx0, cx1, dx,
                          dy, wrap, xaxis, yaxis);
}

extern "C" int sc_curvature(sc_ctx* ctx, double cc, double sc2, double ss, float* out) {
    if (!ctx || !out) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int rc = launch_curv_alpha(ctx, (float)cc, (float)sc2, (float)ss);
    if (rc) return rc;
    SC_HIP(ctx, hipMemcpyAsync(out, ctx->curv.p, sizeof(float) * (size_t)ctx->g.ly * ctx->g.lx,
                               hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SC_OK;
}

extern "C" int sc_curvature_f64(sc_ctx* ctx, double cos2, double sin_a, double cos_a, double sin2,
                               double* out) {
    if (!ctx || !out) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * (size_t)ctx->g.ly * ctx->g.lx;
    int rc = sc_ensure(ctx, ctx->res, bytes);        // (the result planes' buffer: nothing else is live here)
    if (rc) return rc;
    rc = launch_curv_f64(ctx, cos2, sin_a, cos_a, sin2, (double*)ctx->res.p);
    if (rc) return rc;
    SC_HIP(ctx, hipMemcpyAsync(out, ctx->res.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SC_OK;
}

// ---------------------------------------------------------------------------
// generic plugin windows
// ---------------------------------------------------------------------------
extern "C" int sc_upload_window(sc_ctx* ctx, const double* w, int h, int wd, int* slot) {
    if (!ctx || !w || h <= 0 || wd <= 0 || !slot) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    size_t n = (size_t)h * wd;
    std::vector<float> wf(n);
    std::vector<uint8_t> wm(n);
    double l1 = 0.0;
    for (size_t i = 0; i < n; ++i) {
        wf[i] = (float)w[i];
        wm[i] = (w[i] != 0.0) ? 1 : 0;
        l1 += fabs(w[i]);
    }
    WindowSlot s;
    s.l1 = l1;
    s.h = h;
    s.wd = wd;
    SC_HIP(ctx, hipMalloc((void**)&s.w, n * sizeof(float)));
    SC_HIP(ctx, hipMalloc((void**)&s.m, n));
    SC_HIP(ctx, hipMalloc((void**)&s.w64, n * sizeof(double)));      // (the float64 scorers read the window as uploaded)
    SC_HIP(ctx, hipMemcpy(s.w, wf.data(), n * sizeof(float), hipMemcpyHostToDevice));
    SC_HIP(ctx, hipMemcpy(s.m, wm.data(), n, hipMemcpyHostToDevice));
    SC_HIP(ctx, hipMemcpy(s.w64, w, n * sizeof(double), hipMemcpyHostToDevice));
    ctx->windows.push_back(s);
    *slot = (int)ctx->windows.size() - 1;
    return SC_OK;
}

extern "C" int sc_set_masks(sc_ctx* ctx, int slot, const uint8_t* limits, const uint8_t* err) {
    if (!ctx || slot < 0 || slot >= (int)ctx->windows.size()) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    WindowSlot& s = ctx->windows[slot];
    size_t n = (size_t)ctx->g.ny * ctx->g.nx;
    const uint8_t* src[2] = {limits, err};
    uint8_t** dst[2] = {&s.mask_lim, &s.mask_err};
    for (int k = 0; k < 2; ++k) {
        if (*dst[k]) {
            SC_HIP(ctx, hipFree(*dst[k]));
            *dst[k] = nullptr;
        }
        if (src[k]) {
            SC_HIP(ctx, hipMalloc((void**)dst[k], n));
            SC_HIP(ctx, hipMemcpy(*dst[k], src[k], n, hipMemcpyHostToDevice));
        }
    }
    return SC_OK;
}

// ---------------------------------------------------------------------------
// the hot path
// ---------------------------------------------------------------------------
// compare()'s start state (core.py:222-225) in ONE launch: the record (snr 0, amp 0, no id), the resolution
// statistic, and the scratch records of a split row pass (a share left by an earlier search must not score
// against the new record).  Five memsets before: a fifth of a millisecond per five-scale C5 step in fills and gaps.
__global__ void __launch_bounds__(256)
k_reset_best(float* __restrict__ snr, float* __restrict__ amp, uint32_t* __restrict__ id, size_t nc,
             float* __restrict__ s2, size_t n2, unsigned long long* __restrict__ stats) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    for (size_t i = i0; i < nc; i += step) { snr[i] = 0.f; amp[i] = 0.f; id[i] = SC_ID_NONE; }
    for (size_t i = i0; i < n2; i += step) s2[i] = 0.f;
    if (i0 < 2) stats[i0] = 0ull;
}

extern "C" int sc_reset_best(sc_ctx* ctx) {
    if (!ctx) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    size_t nc = (size_t)(ctx->g.cy1 - ctx->g.cy0) * (ctx->g.cx1 - ctx->g.cx0);
    int rc = sc_ensure(ctx, ctx->res_stats, 2 * sizeof(unsigned long long));
    if (rc) return rc;
    const size_t n2 = ctx->split_s.p ? ctx->split_s.cap / sizeof(float) : 0;
    const unsigned blocks = (unsigned)std::min<size_t>((std::max(nc, n2) + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_reset_best, dim3(blocks), dim3(256), 0, ctx->stream, (float*)ctx->best_snr.p,
                       (float*)ctx->best_amp.p, (uint32_t*)ctx->best_id.p, nc, (float*)ctx->split_s.p, n2,
                       (unsigned long long*)ctx->res_stats.p);
    SC_HIP(ctx, hipGetLastError());
    if (ctx->near.p) SC_HIP(ctx, hipMemsetAsync(ctx->near.p, 0, ctx->near.cap, ctx->stream));
    if (ctx->near_ev.p) SC_HIP(ctx, hipMemsetAsync(ctx->near_ev.p, 0, 16, ctx->stream));
    ctx->patch_n = 0;
    return SC_OK;
}

int sc_near_buffers(sc_ctx* ctx, unsigned long long** ev_count, uint32_t** ev, unsigned long long* ev_cap) {
    const size_t nc = (size_t)(ctx->g.cy1 - ctx->g.cy0) * (ctx->g.cx1 - ctx->g.cx0);
    const bool fresh = ctx->near.cap < nc;
    int rc = sc_ensure(ctx, ctx->near, nc);
    if (rc) return rc;
    if (fresh) SC_HIP(ctx, hipMemsetAsync(ctx->near.p, 0, ctx->near.cap, ctx->stream));
    // the event list: two per core cell or a million, whichever is more (12 bytes each); counter in front
    const unsigned long long cap = std::max<unsigned long long>(2ull * nc, 1ull << 20);
    const bool fresh_ev = ctx->near_ev.cap < 16 + 4 * SC_EVENT_WORDS * cap;
    if ((rc = sc_ensure(ctx, ctx->near_ev, 16 + 4 * SC_EVENT_WORDS * cap))) return rc;
    if (fresh_ev) SC_HIP(ctx, hipMemsetAsync(ctx->near_ev.p, 0, 16, ctx->stream));
    *ev_count = (unsigned long long*)ctx->near_ev.p;
    *ev = (uint32_t*)((char*)ctx->near_ev.p + 16);
    *ev_cap = (ctx->near_ev.cap - 16) / (4 * SC_EVENT_WORDS);
    ctx->near_w_used = ctx->near_w;
    return SC_OK;
}

extern "C" int sc_get_near_ties(sc_ctx* ctx, uint8_t* out) {
    if (!ctx || !out) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nc = (size_t)(ctx->g.cy1 - ctx->g.cy0) * (ctx->g.cx1 - ctx->g.cx0);
    if (!ctx->near.p || ctx->near.cap < nc) {        // no search has run with the option on: nothing flagged
        memset(out, 0, nc);
        return SC_OK;
    }
    SC_HIP(ctx, hipMemcpyAsync(out, ctx->near.p, nc, hipMemcpyDeviceToHost, ctx->stream));
    return sc_sync(ctx);
}

extern "C" int sc_get_near_events(sc_ctx* ctx, uint32_t* events, long long capacity, long long* n_events) {
    if (!ctx || !n_events || capacity < 0 || (capacity > 0 && !events)) return SC_ERR_INVALID;
    *n_events = 0;
    if (!ctx->near_ev.p) return SC_OK;                   // no FFT search has run with the option on
    SC_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long n = 0;
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SC_HIP(ctx, hipMemcpy(&n, ctx->near_ev.p, sizeof(n), hipMemcpyDeviceToHost));
    *n_events = (long long)n;
    const unsigned long long held = std::min<unsigned long long>(n, (ctx->near_ev.cap - 16) / (4 * SC_EVENT_WORDS));
    const unsigned long long take = std::min<unsigned long long>(held, (unsigned long long)capacity);
    if (n > held)                                        // the device list overflowed: events were dropped - said, not left to the caller's arithmetic
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_get_near_events: the event list overflowed (%llu near-ties, room for %llu)", n, held);
    if (held > (unsigned long long)capacity) return SC_OK;                  // the caller asks again with room (*n_events says how much)
    if (take) SC_HIP(ctx, hipMemcpy(events, (const char*)ctx->near_ev.p + 16, 4 * SC_EVENT_WORDS * take, hipMemcpyDeviceToHost));
    return SC_OK;
}

// shared by sc_score_cells_f64 (tsel = nullptr: every cell against every template) and sc_score_pairs_f64
static int score_f64(sc_ctx* ctx, const int32_t* cells, const int32_t* tsel, int m, double* amp, double* snr, const char* who) {
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    const int n = ctx->last_batch;
    if (n <= 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: no search has run in this context", who);
    SC_HIP(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < m; ++k) {
        if (cells[2 * k] < 0 || cells[2 * k] >= ctx->g.ny || cells[2 * k + 1] < 0 || cells[2 * k + 1] >= ctx->g.nx)
            return sc_fail(ctx, SC_ERR_INVALID, "%s: cell %d outside the DEM", who, k);
        if (tsel && (tsel[k] < 0 || tsel[k] >= n))
            return sc_fail(ctx, SC_ERR_INVALID, "%s: pair %d names template %d of %d", who, k, tsel[k], n);
    }
    const size_t nout = tsel ? (size_t)m : (size_t)m * n;
    int rc = sc_ensure(ctx, ctx->score, sizeof(int32_t) * 3 * (size_t)m + 16 + sizeof(double) * 2 * nout);
    if (rc) return rc;
    double* d_amp = (double*)ctx->score.p;
    double* d_snr = d_amp + nout;
    int* d_cells = (int*)(d_snr + nout);
    int* d_tsel = tsel ? d_cells + 2 * (size_t)m : nullptr;
    SC_HIP(ctx, hipMemcpyAsync(d_cells, cells, sizeof(int32_t) * 2 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    if (tsel) SC_HIP(ctx, hipMemcpyAsync(d_tsel, tsel, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    // (grid.y is limited to 65535: the templates of a search are at most a few thousand)
    if (!tsel && n > 65535) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %d templates", who, n);
    if ((rc = launch_score_f64(ctx, d_cells, d_tsel, m, n, d_amp, d_snr))) return rc;
    SC_HIP(ctx, hipMemcpyAsync(amp, d_amp, sizeof(double) * nout, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(snr, d_snr, sizeof(double) * nout, hipMemcpyDeviceToHost, ctx->stream));
    return sc_sync(ctx);
}

extern "C" int sc_score_pairs_f64(sc_ctx* ctx, const int32_t* cells, const int32_t* templates, int m, double* amp, double* snr) {
    if (!ctx || !cells || !templates || m <= 0 || !amp || !snr) return SC_ERR_INVALID;
    return score_f64(ctx, cells, templates, m, amp, snr, "sc_score_pairs_f64");
}

extern "C" int sc_score_cells_f64(sc_ctx* ctx, const int32_t* cells, int m, int n_templates, double* amp, double* snr) {
    if (!ctx || !cells || m <= 0 || !amp || !snr) return SC_ERR_INVALID;
    // (the caller sized amp / snr for m x n_templates values: it must be the number this context will write)
    if (n_templates != ctx->last_batch)
        return sc_fail(ctx, SC_ERR_INVALID, "sc_score_cells_f64: the caller expects %d templates, the last search held %d",
                       n_templates, ctx->last_batch);
    return score_f64(ctx, cells, nullptr, m, amp, snr, "sc_score_cells_f64");
}

extern "C" int sc_get_resolution_stats(sc_ctx* ctx, long long* wins, long long* near_floor) {
    if (!ctx || !wins || !near_floor) return SC_ERR_INVALID;
    *wins = *near_floor = 0;
    if (!ctx->res_stats.p) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long h[2] = {0, 0};
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SC_HIP(ctx, hipMemcpy(h, ctx->res_stats.p, sizeof(h), hipMemcpyDeviceToHost));
    *wins = (long long)h[0];
    *near_floor = (long long)h[1];
    return SC_OK;
}

static int check_templates(sc_ctx* ctx, const sc_template* t, int n, const sc_plan* plan) {
    const Geom& g = ctx->g;
    for (int i = 0; i < n; ++i) {
        const sc_template& s = t[i];
        if (s.kind < SC_KIND_SCARP || s.kind > SC_KIND_WINDOW)
            return sc_fail(ctx, SC_ERR_INVALID, "template %d: unknown kind %d", i, s.kind);
        if (s.pmax < s.pmin || s.qmax < s.qmin)
            return sc_fail(ctx, SC_ERR_INVALID, "template %d: empty support box", i);
        // support cells must exist on the ny x nx template grid
        if (g.ny / 2 + s.pmin < 0 || g.ny / 2 + s.pmax >= g.ny ||
            g.nx / 2 + s.qmin < 0 || g.nx / 2 + s.qmax >= g.nx)
            return sc_fail(ctx, SC_ERR_INVALID, "template %d: support box leaves the grid", i);
        if (s.kind == SC_KIND_WINDOW) {
            if (s.window < 0 || s.window >= (int)ctx->windows.size())
                return sc_fail(ctx, SC_ERR_INVALID, "template %d: bad window slot", i);
            const WindowSlot& w = ctx->windows[s.window];
            if (w.h != s.pmax - s.pmin + 1 || w.wd != s.qmax - s.qmin + 1)
                return sc_fail(ctx, SC_ERR_INVALID, "template %d: window size mismatch", i);
        }
        if (plan->method == SC_METHOD_DIRECT && !direct_window_fits(s.qmax - s.qmin + 1))
            return sc_fail(ctx, SC_ERR_UNSUPPORTED, "template %d: a %d-cell wide window exceeds the "
                           "real-space kernel's LDS slab; use SC_METHOD_FFT", i, s.qmax - s.qmin + 1);
        if (plan->method == SC_METHOD_FFT) {
            if (s.pmax > plan->Py || s.qmax > plan->Qx ||
                plan->Py - s.pmin > plan->Ty - plan->Vy + (plan->circ_y ? plan->Ty : 0) ||
                plan->Qx - s.qmin > plan->Tx - plan->Vx + (plan->circ_x ? plan->Tx : 0))
                return sc_fail(ctx, SC_ERR_INVALID, "template %d: support exceeds the plan", i);
            if (s.pmax - s.pmin >= plan->Ty || s.qmax - s.qmin >= plan->Tx)
                return sc_fail(ctx, SC_ERR_INVALID, "template %d: support exceeds the tile", i);
        }
    }
    return SC_OK;
}

// One descriptor as the device's table entry (offsets into the per-chunk window buffers: sc_match_plan's, filled by match_impl)
static void templ_from_descriptor(const sc_ctx* ctx, const sc_template& s, TemplDev& d, double* sums2, double* wl1) {
    const Geom& g = ctx->g;
    d.kind = s.kind; d.flags = s.flags;
    d.cos_a = s.cos_a; d.sin_a = s.sin_a; d.c = s.c; d.d = s.d;
    d.p0 = s.p0; d.p1 = s.p1;
    d.ilo = s.ilo; d.ihi = s.ihi; d.jlo = s.jlo; d.jhi = s.jhi;
    if (s.flags & SC_FLAG_NO_LIMITS) { d.ilo = 0; d.ihi = g.ny - 1; d.jlo = 0; d.jhi = g.nx - 1; }
    d.pmin = s.pmin; d.pmax = s.pmax; d.qmin = s.qmin; d.qmax = s.qmax;
    d.id = s.id;
    d.wh = s.pmax - s.pmin + 1;
    d.ww = s.qmax - s.qmin + 1;
    d.win_off = 0;
    d.mask_lim = nullptr; d.mask_err = nullptr;
    if (s.kind == SC_KIND_WINDOW) {
        d.mask_lim = ctx->windows[s.window].mask_lim;
        d.mask_err = ctx->windows[s.window].mask_err;
        sums2[0] = s.p0;
        sums2[1] = s.p1;
        *wl1 = ctx->windows[s.window].l1;
    }
}

// What the float64 scorers need of a search beyond TemplDev: every template's window slot and orientation mix
static void keep_f64_side(sc_ctx* ctx, const sc_template* t, int n) {
    ctx->h_wslot.assign(n, -1);
    ctx->h_mix.assign(3 * (size_t)n, 0.0);
    ctx->templ_windows = false;
    for (int j = 0; j < n; ++j) {
        if (t[j].kind == SC_KIND_WINDOW) ctx->h_wslot[j] = t[j].window;
        ctx->h_mix[3 * (size_t)j] = t[j].cc;
        ctx->h_mix[3 * (size_t)j + 1] = t[j].sc2;
        ctx->h_mix[3 * (size_t)j + 2] = t[j].ss;
        ctx->templ_windows = ctx->templ_windows || t[j].kind == SC_KIND_WINDOW;
    }
}

// The descriptors of a whole search as the template table the float64 scorer reads, without matching them
// (sc_settle_pairs: a rank of an orientation-sharded search settles candidates of templates other ranks matched)
int sc_load_templates(sc_ctx* ctx, const sc_template* t, int n) {
    sc_plan plan{};
    plan.method = -1;                            // (neither path's support limits: the float64 scorer has none)
    int rc = check_templates(ctx, t, n, &plan);
    if (rc) return rc;
    if (ctx->async_in_flight) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->async_in_flight = false;
    }
    std::vector<TemplDev>& h = ctx->h_templ;
    h.assign(n, TemplDev{});
    ctx->h_sums.assign(2 * (size_t)n, 0.0);
    ctx->h_wl1.assign(n, 0.0);
    for (int j = 0; j < n; ++j) templ_from_descriptor(ctx, t[j], h[j], &ctx->h_sums[2 * (size_t)j], &ctx->h_wl1[j]);
    keep_f64_side(ctx, t, n);
    if ((rc = sc_ensure(ctx, ctx->templ, sizeof(TemplDev) * n))) return rc;
    ctx->async_in_flight = true;
    SC_HIP(ctx, hipMemcpyAsync(ctx->templ.p, h.data(), sizeof(TemplDev) * n, hipMemcpyHostToDevice, ctx->stream));
    ctx->last_batch = n;
    return SC_OK;
}

// The curvature of a chunk, mixed for its nb orientations - and, on the FFT path, transformed - unless it is there
// already: in the chunk's kept-spectra slots (`slot0` >= 0: the search keeps them, option "spectra_mb"), or, for a single
// orientation, in plane 0 from the chunk before (`cur`: what plane 0 holds, while `have_curv`).
struct CurvState {
    double cur[3] = {0, 0, 0};
    bool have_curv = false;
};
static int chunk_curvature(sc_ctx* ctx, const sc_template* t, const MatchChunk& c, bool fft, const FftGeom& fg, int slot0,
                           CurvState& st) {
    const bool keep = slot0 >= 0;
    bool hit = keep;
    if (keep) {
        ctx->uc_off = (size_t)slot0 * ctx->spec_uc_stride;
        ctx->norms_off = (size_t)slot0 * ctx->spec_norm_stride;
    }
    for (int b = 0; b < c.nb && hit; ++b) {
        const sc_template& sb = t[c.first + b * c.n];
        const double* k = &ctx->spec_key[3 * (size_t)(slot0 + b)];
        hit = k[0] == sb.cc && k[1] == sb.sc2 && k[2] == sb.ss;
    }
    if (hit) {
        st.have_curv = false;                     // (the curvature plane itself was not rebuilt)
        return SC_OK;
    }
    const sc_template& s0 = t[c.first];
    if (c.nb > 1 || !st.have_curv || s0.cc != st.cur[0] || s0.sc2 != st.cur[1] || s0.ss != st.cur[2]) {
        float coef[SC_MAX_ORIENT][3];
        for (int b = 0; b < c.nb; ++b) {
            const sc_template& sb = t[c.first + b * c.n];
            coef[b][0] = (float)sb.cc; coef[b][1] = (float)sb.sc2; coef[b][2] = (float)sb.ss;
        }
        // FFT tiles: the orientations' curvature is mixed from the stencil planes inside the forward row
        // kernel (no plane written and read back; option "variant" 17: the separate k_curv_alpha pass, for the
        // cross-check - same bits); the real-space kernel reads the plane(s)
        const bool fused = fft && ctx->variant != 17;
        int rc = SC_OK;
        if (!fused) rc = c.nb > 1 ? launch_curv_alpha_batch(ctx, coef, c.nb) : launch_curv_alpha(ctx, coef[0][0], coef[0][1], coef[0][2]);
        if (rc) return rc;
        if (fft && (rc = fft_forward_curv(ctx, fg, c.nb, fused ? coef : nullptr))) return rc;
        st.cur[0] = s0.cc; st.cur[1] = s0.sc2; st.cur[2] = s0.ss;
        st.have_curv = c.nb == 1;                 // (a batch: plane 0 no longer belongs to a single run)
    }
    for (int b = 0; b < c.nb && keep; ++b) {
        const sc_template& sb = t[c.first + b * c.n];
        double* k = &ctx->spec_key[3 * (size_t)(slot0 + b)];
        k[0] = sb.cc; k[1] = sb.sc2; k[2] = sb.ss;
    }
    return SC_OK;
}

// A search: validate, plan (sc_match_plan.h: runs, chunks, offsets and slots are decided there), upload, and launch
// chunk after chunk.
static int match_impl(sc_ctx* ctx, const sc_template* t, int n, const sc_plan* plan,
                      bool to_maps) {
    if (!ctx || !t || !plan || n <= 0) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    if (plan->method != SC_METHOD_DIRECT && plan->method != SC_METHOD_FFT)
        return sc_fail(ctx, SC_ERR_INVALID, "unknown method %d", plan->method);
    int rc = check_templates(ctx, t, n, plan);
    if (rc) return rc;
    if (!to_maps) ctx->patch_n = 0;            // (the record moves on: what sc_settle_exact patched no longer describes it)
    const Geom& g = ctx->g;
    const bool fft = plan->method == SC_METHOD_FFT;
    const MatchPlanRefusal bad = sc_match_plan_check(*plan, g.ny, g.nx, g.wrap != 0, g.cy1 - g.cy0, g.cx1 - g.cx0);
    if (bad.err) return sc_fail(ctx, bad.err, "%s", bad.msg);
    FftGeom fg{};
    const int group = std::max(1, plan->group);
    if (fft) {
        fg.Ty = plan->Ty; fg.Tx = plan->Tx; fg.Vy = plan->Vy; fg.Vx = plan->Vx;
        fg.nty = plan->nty; fg.ntx = plan->ntx; fg.circ_y = plan->circ_y;
        fg.circ_x = plan->circ_x; fg.Py = plan->Py; fg.Qx = plan->Qx;
        fg.ntiles = fg.nty * fg.ntx;
    }
    if (to_maps) {
        size_t nc = (size_t)(g.cy1 - g.cy0) * (g.cx1 - g.cx0);
        if ((rc = sc_ensure(ctx, ctx->map_amp, sizeof(float) * nc))) return rc;
        if ((rc = sc_ensure(ctx, ctx->map_snr, sizeof(float) * nc))) return rc;
    }

    // (the context's own vectors: the uploads below are asynchronous and nothing waits for them before
    //  the launches; the stream was drained at the end of the previous call, so they are free to reuse -
    //  after an sc_match_async without sc_sync it is drained here)
    if (ctx->async_in_flight) {
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->async_in_flight = false;
    }
    std::vector<TemplDev>& h = ctx->h_templ;
    std::vector<double>&sums = ctx->h_sums, &wl1 = ctx->h_wl1;
    std::vector<unsigned char>& masked = ctx->h_masked;
    h.assign(n, TemplDev{});
    sums.assign(2 * (size_t)n, 0.0);
    wl1.assign(n, 0.0);
    masked.assign(n, 0);
    for (int j = 0; j < n; ++j) {
        templ_from_descriptor(ctx, t[j], h[j], &sums[2 * (size_t)j], &wl1[j]);
        masked[j] = h[j].mask_lim != nullptr || h[j].mask_err != nullptr;
    }
    MatchPlanIn in{};
    in.t = t; in.n = n; in.masked = masked.data();
    in.method = plan->method; in.to_maps = to_maps;
    in.ch = g.cy1 - g.cy0; in.cw = g.cx1 - g.cx0; in.oy = g.oy; in.ox = g.ox; in.dx = ctx->dx;
    in.route = fft_route_in(ctx, fg, 1);
    in.route.group = group;
    in.spectra = ctx->spec_mb > 0.0;
    const MatchPlan mp = sc_match_plan(in);
    for (int j = 0; j < n; ++j) {
        h[j].win_off = mp.win_off[j]; h[j].dwin_off = mp.dwin_off[j];
        h[j].dpitch = mp.dpitch[j]; h[j].span_off = mp.span_off[j];
    }
    if (fft && (rc = fft_prepare(ctx, fg, std::min(n, std::max(SC_MAX_GROUP, mp.max_batch_templ)), group, mp.nb_max, mp.n_slots)))
        return rc;
    const bool keep = fft && ctx->spec_slots > 0;
    templ_cache_use(ctx, nullptr, fg, 0);
    if (fft) templ_cache_budget(ctx);
    if ((rc = sc_ensure(ctx, ctx->templ, sizeof(TemplDev) * n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sums, sizeof(double) * 2 * n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->wl1, sizeof(double) * n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->win_w, sizeof(float) * mp.max_cells))) return rc;
    if ((rc = sc_ensure(ctx, ctx->win_m, mp.max_cells))) return rc;
    if (!fft) {
        if ((rc = sc_ensure(ctx, ctx->curv, sizeof(float) * (size_t)g.ly * g.lx * mp.nb_max))) return rc;
        if ((rc = sc_ensure(ctx, ctx->dwin, sizeof(float2) * std::max<size_t>(mp.max_dcells, 4)))) return rc;
        if ((rc = sc_ensure(ctx, ctx->spans, sizeof(int4) * std::max<size_t>(mp.max_spans, 1)))) return rc;
    }
    // from here on the context's host vectors are the source of copies in flight: whatever way this call ends
    // (a launch failure or an allocation failing in a later chunk returns without draining the stream), the
    // next call's prologue waits before it reuses them; sc_sync, at the end of every successful synchronous
    // call, clears the flag
    ctx->async_in_flight = true;
    SC_HIP(ctx, hipMemcpyAsync(ctx->templ.p, h.data(), sizeof(TemplDev) * n,
                               hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(ctx->sums.p, sums.data(), sizeof(double) * 2 * n,
                               hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(ctx->wl1.p, wl1.data(), sizeof(double) * n,
                               hipMemcpyHostToDevice, ctx->stream));
    ctx->last_batch = n;
    keep_f64_side(ctx, t, n);

    CurvState curv;
    for (const MatchChunk& c : mp.chunks) {
        const int n_all = c.nb * c.n;
        if ((rc = chunk_curvature(ctx, t, c, fft, fg, keep ? mp.slot_of[c.run0] : -1, curv))) return rc;
        for (int j = c.first; j < c.first + n_all; ++j) {
            if (t[j].kind != SC_KIND_WINDOW) continue;
            const WindowSlot& w = ctx->windows[t[j].window];
            size_t cells = (size_t)w.h * w.wd;
            SC_HIP(ctx, hipMemcpyAsync((float*)ctx->win_w.p + h[j].win_off, w.w,
                                       cells * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
            SC_HIP(ctx, hipMemcpyAsync((uint8_t*)ctx->win_m.p + h[j].win_off, w.m, cells,
                                       hipMemcpyDeviceToDevice, ctx->stream));
        }
        // The template forward chain (k_windows, the row transform, the column transform and split) - unless the
        // chunk's planes and sums wait in the template cache from an earlier search: then nothing of it is launched
        // (nothing downstream reads win_w / win_m on the FFT path; the real-space path is never cached).  A miss runs
        // the chain as ever, writing into the new entry's planes: no copy.
        bool hit = false;
        TemplEntry* e = fft ? templ_cache_entry(ctx, t, c, fg, &hit) : nullptr;
        templ_cache_use(ctx, e, fg, n_all);
        if (!hit) {
            rc = launch_windows(ctx, c.first, n_all, c.wh, c.ww);
            if (!rc && fft) rc = fft_forward_templates(ctx, fg, c.first, n_all, c.parity);
            if (!rc && e) rc = templ_cache_sums(ctx, e, fg, c.first, n_all, true);
        } else {
            rc = templ_cache_sums(ctx, e, fg, c.first, n_all, false);
        }
        if (rc) {
            templ_cache_use(ctx, nullptr, fg, 0);
            if (e && !hit) ctx->tc.discard(e);       // (half-filled planes must not be found again)
            return rc;
        }
        if (!fft) rc = launch_direct(ctx, c.first, c.n, to_maps, c.nb, c.wh, c.ww, c.long_runs);
        else rc = fft_inverse_fold(ctx, fg, c.first, c.n, group, to_maps, c.full, c.parity, c.nb);
        templ_cache_use(ctx, nullptr, fg, 0);
        if (rc) return rc;
    }
    return SC_OK;
}

extern "C" int sc_match_async(sc_ctx* ctx, const sc_template* t, int n, const sc_plan* plan) {
    int rc = match_impl(ctx, t, n, plan, false);
    if (ctx) ctx->async_in_flight = true;
    return rc;
}

extern "C" int sc_sync(sc_ctx* ctx) {
    if (!ctx) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->async_in_flight = false;
    sc_prof_collect(ctx);
    return SC_OK;
}

extern "C" int sc_match(sc_ctx* ctx, const sc_template* t, int n, const sc_plan* plan) {
    int rc = match_impl(ctx, t, n, plan, false);
    if (rc) return rc;
    return sc_sync(ctx);
}

extern "C" int sc_match_template(sc_ctx* ctx, const sc_template* t, const sc_plan* plan,
                                 float* amp, float* snr) {
    if (!amp || !snr) return SC_ERR_INVALID;
    int rc = match_impl(ctx, t, 1, plan, true);
    if (rc) return rc;
    size_t nc = (size_t)(ctx->g.cy1 - ctx->g.cy0) * (ctx->g.cx1 - ctx->g.cx0);
    SC_HIP(ctx, hipMemcpyAsync(amp, ctx->map_amp.p, sizeof(float) * nc, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(snr, ctx->map_snr.p, sizeof(float) * nc, hipMemcpyDeviceToHost, ctx->stream));
    return sc_sync(ctx);
}

extern "C" int sc_forget_templates(sc_ctx* ctx) {
    if (!ctx) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    ctx->tc.clear();
    return SC_OK;
}

extern "C" int sc_templ_cache_info(sc_ctx* ctx, long long* hits, long long* misses, long long* entries, long long* bytes,
                                   long long* evictions) {
    if (!ctx) return SC_ERR_INVALID;
    const TemplCacheStats s = ctx->tc.stats();
    if (hits) *hits = s.hits;
    if (misses) *misses = s.misses;
    if (entries) *entries = s.entries;
    if (bytes) *bytes = s.bytes;
    if (evictions) *evictions = s.evictions;
    return SC_OK;
}

extern "C" int sc_get_best(sc_ctx* ctx, float* amp, float* snr, uint32_t* id) {
    if (!ctx || !amp || !snr || !id) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    size_t nc = (size_t)(ctx->g.cy1 - ctx->g.cy0) * (ctx->g.cx1 - ctx->g.cx0);
    SC_HIP(ctx, hipMemcpyAsync(amp, ctx->best_amp.p, sizeof(float) * nc, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(snr, ctx->best_snr.p, sizeof(float) * nc, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(id, ctx->best_id.p, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost, ctx->stream));
    return sc_sync(ctx);
}

// (amp, snr, id) float32 record -> the reference's four float64 planes
__global__ void __launch_bounds__(256)
k_result(const float* __restrict__ amp, const float* __restrict__ snr,
         const uint32_t* __restrict__ id, const double* __restrict__ par,
         const double* __restrict__ ang, uint32_t n_ids, size_t nc, double* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nc; i += (size_t)gridDim.x * 256) {
        const uint32_t t = id[i];
        const bool won = t < n_ids;                 // SC_ID_NONE is larger than any id
        out[i] = (double)amp[i];
        out[nc + i] = won ? par[t] : 0.0;
        out[2 * nc + i] = won ? ang[t] : 0.0;
        out[3 * nc + i] = (double)snr[i];
    }
}

// k_result on any record of n cells (sc_gather_result converts the other ranks' records at the root)
int sc_launch_result(sc_ctx* ctx, const float* amp, const float* snr, const uint32_t* id, const double* tab_par,
                     const double* tab_ang, int n_ids, size_t n, double* planes) {
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(k_result, dim3(blocks), dim3(256), 0, ctx->stream, amp, snr, id, tab_par, tab_ang,
                       (uint32_t)n_ids, n, planes);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

// the record of this context's core as four float64 planes in ctx->res (device)
int sc_result_planes(sc_ctx* ctx, const double* param_of_id, const double* angle_of_id, int n_ids,
                     double** planes_out, size_t* nc_out) {
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nc = (size_t)(ctx->g.cy1 - ctx->g.cy0) * (ctx->g.cx1 - ctx->g.cx0);
    int rc = sc_ensure(ctx, ctx->res, sizeof(double) * (4 * nc + 2 * (size_t)n_ids));
    if (rc) return rc;
    double* planes = (double*)ctx->res.p;
    double* tab = planes + 4 * nc;
    SC_HIP(ctx, hipMemcpyAsync(tab, param_of_id, sizeof(double) * n_ids, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(tab + n_ids, angle_of_id, sizeof(double) * n_ids, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sc_launch_result(ctx, (const float*)ctx->best_amp.p, (const float*)ctx->best_snr.p,
                               (const uint32_t*)ctx->best_id.p, tab, tab + n_ids, n_ids, nc, planes)))
        return rc;
    if (ctx->patch_n && (rc = sc_apply_patches(ctx, tab, tab + n_ids, n_ids, nc, planes))) return rc;
    *planes_out = planes;
    *nc_out = nc;
    return SC_OK;
}

extern "C" int sc_get_result(sc_ctx* ctx, const double* param_of_id, const double* angle_of_id,
                             int n_ids, double* out) {
    if (!ctx || !param_of_id || !angle_of_id || n_ids <= 0 || !out) return SC_ERR_INVALID;
    double* planes = nullptr;
    size_t nc = 0;
    int rc = sc_result_planes(ctx, param_of_id, angle_of_id, n_ids, &planes, &nc);
    if (rc) return rc;
    SC_HIP(ctx, hipMemcpyAsync(out, planes, sizeof(double) * 4 * nc, hipMemcpyDeviceToHost, ctx->stream));
    return sc_sync(ctx);
}

extern "C" int sc_get_template_sums(sc_ctx* ctx, int n, double* n_out, double* ts_out) {
    if (!ctx || !n_out || !ts_out || n <= 0 || n > ctx->last_batch) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> h(2 * (size_t)n);
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SC_HIP(ctx, hipMemcpy(h.data(), ctx->sums.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        n_out[i] = h[2 * (size_t)i] + SC_EPS;
        ts_out[i] = h[2 * (size_t)i + 1];
    }
    return SC_OK;
}

// ---------------------------------------------------------------------------
// nodata fill (pre-step of the matcher: DEMGrid._fill_nodata)
// ---------------------------------------------------------------------------
extern "C" int sc_fill_nodata(sc_ctx* ctx, double* z, int ny, int nx, double max_search_distance,
                              int smoothing_iterations, long long* remaining) {
    if (!ctx || !z || ny <= 0 || nx <= 0 || !(max_search_distance >= 0.0) || smoothing_iterations < 0)
        return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ny * nx;
    int rc;
    if ((rc = sc_ensure(ctx, ctx->fill[0], sizeof(double) * n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->fill[1], sizeof(double) * n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->fill[2], sizeof(int) * 2 * n + 16))) return rc;      // up | down, contiguous
    if ((rc = sc_ensure(ctx, ctx->fill[3], 16))) return rc;
    SC_HIP(ctx, hipMemcpyAsync(ctx->fill[0].p, z, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    int* up = (int*)ctx->fill[2].p;
    rc = launch_fill_nodata(ctx, (double*)ctx->fill[0].p, (double*)ctx->fill[1].p, up, up + n, ny, nx,
                            max_search_distance, smoothing_iterations, (unsigned long long*)ctx->fill[3].p);
    if (rc) return rc;
    unsigned long long left = 0;
    SC_HIP(ctx, hipMemcpyAsync(z, ctx->fill[0].p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(&left, ctx->fill[3].p, sizeof(left), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (remaining) *remaining = (long long)left;
    return SC_OK;
}

// ---------------------------------------------------------------------------
// compare() on host results
// ---------------------------------------------------------------------------
extern "C" int sc_compare_begin(sc_ctx* ctx, int ny, int nx) {
    if (!ctx || ny <= 0 || nx <= 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    size_t n = (size_t)ny * nx;
    int rc;
    for (int k = 0; k < 4; ++k) {
        if ((rc = sc_ensure(ctx, ctx->cmp[k], sizeof(double) * n))) return rc;
        SC_HIP(ctx, hipMemsetAsync(ctx->cmp[k].p, 0, sizeof(double) * n, ctx->stream));
    }
    for (int k = 0; k < 2; ++k)
        if ((rc = sc_ensure(ctx, ctx->cmp_in[k], sizeof(double) * n))) return rc;
    ctx->cmp_n = n;
    return SC_OK;
}

static int compare_fold_impl(sc_ctx* ctx, const double* amp, const double* snr,
                             const double* age_p, const double* angle_p, double age, double angle) {
    if (!ctx || !amp || !snr || ctx->cmp_n == 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    size_t bytes = sizeof(double) * ctx->cmp_n;
    const bool planes = age_p && angle_p;
    SC_HIP(ctx, hipMemcpyAsync(ctx->cmp_in[0].p, amp, bytes, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(ctx->cmp_in[1].p, snr, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (planes) {
        int rc;
        for (int k = 2; k < 4; ++k)
            if ((rc = sc_ensure(ctx, ctx->cmp_in[k], bytes))) return rc;
        SC_HIP(ctx, hipMemcpyAsync(ctx->cmp_in[2].p, age_p, bytes, hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipMemcpyAsync(ctx->cmp_in[3].p, angle_p, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    int rc = launch_compare_fold(ctx, age, angle, planes);
    if (rc) return rc;
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SC_OK;
}

extern "C" int sc_compare_fold(sc_ctx* ctx, const double* amp, const double* snr,
                               double age, double angle) {
    return compare_fold_impl(ctx, amp, snr, nullptr, nullptr, age, angle);
}

extern "C" int sc_compare_fold_planes(sc_ctx* ctx, const double* amp, const double* age,
                                      const double* angle, const double* snr) {
    if (!age || !angle) return SC_ERR_INVALID;
    return compare_fold_impl(ctx, amp, snr, age, angle, 0.0, 0.0);
}

extern "C" int sc_compare_end(sc_ctx* ctx, double* amp, double* age, double* angle, double* snr) {
    if (!ctx || !amp || !age || !angle || !snr || ctx->cmp_n == 0) return SC_ERR_INVALID;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    size_t bytes = sizeof(double) * ctx->cmp_n;
    double* out[4] = {amp, age, angle, snr};
    for (int k = 0; k < 4; ++k)
        SC_HIP(ctx, hipMemcpyAsync(out[k], ctx->cmp[k].p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cmp_n = 0;
    return SC_OK;
}

// ---------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------
extern "C" int sc_profile(sc_ctx* ctx, int enable) {
    if (!ctx) return SC_ERR_INVALID;
    sc_prof_collect(ctx);
    ctx->prof = enable < 0 ? 0 : enable;
    for (int k = 0; k < SC_K_COUNT; ++k) {
        ctx->k_launches[k] = 0;
        ctx->k_brackets[k] = 0;
        ctx->k_sampled[k] = 0;
        ctx->k_ms[k] = 0.0;
    }
    return SC_OK;
}

extern "C" int sc_profile_get(sc_ctx* ctx, int kernel, long long* launches, double* total_ms) {
    if (!ctx || kernel < 0 || kernel >= SC_K_COUNT) return SC_ERR_INVALID;
    sc_prof_collect(ctx);
    if (launches) *launches = ctx->k_launches[kernel];
    if (total_ms) {
        // sampled mean duration times the number of launches
        double mean = ctx->k_sampled[kernel] ? ctx->k_ms[kernel] / (double)ctx->k_sampled[kernel] : 0.0;
        *total_ms = mean * (double)ctx->k_launches[kernel];
    }
    return SC_OK;
}

extern "C" const char* sc_kernel_name(int kernel) {
    static const char* names[SC_K_COUNT] = {"k_curv", "k_windows", "k_direct", "k_fwd_rows",
                                            "k_fwd_cols", "k_inv_cols", "k_inv_rows", "k_settle", "k_noise", "k_trace", "k_profile"};
    return (kernel >= 0 && kernel < SC_K_COUNT) ? names[kernel] : "?";
}

