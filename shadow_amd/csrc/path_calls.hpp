#pragma once
// path_calls.hpp -- the path calls of the engine: hop counts and explicit routes
// (path_hops.hpp), link loads (link_loads.hpp), path folds (path_fold.hpp), the tie envelope
// (path_ties.hpp), the ECMP link loads (ecmp_loads.hpp), the link loss (link_loss.hpp), the link outages (link_outage.hpp) and the link repricing (link_reprice.hpp), over
// one set of host stages.  What needs no device is path_host.hpp; here are the uploads, the launches and the entry points.  Not a stand-alone
// header: engine.hip includes it once struct shd_route, hip_check, upload, DevBuf and
// shd_route_rows_async are defined.

namespace {

// ---- stages every entry point shares ----
// the block arguments (ld: the row stride of an async call; a blocking call's is nt)
bool block_args_ok(const shd_route* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, int64_t ld) {
    return c && ns >= 0 && nt >= 0 && (!ns || src) && (!nt || tgt) && ld >= nt;
}

bool pair_args_ok(const shd_route* c, const int32_t* pair_src, const int32_t* pair_tgt, int64_t npairs) {
    return c && npairs >= 0 && npairs <= 0x7FFFFFFF && (!npairs || (pair_src && pair_tgt));
}

bool pairs_in_range(const shd_route* c, const int32_t* pair_src, const int32_t* pair_tgt, int np) {
    for (int k = 0; k < np; k++)
        if (pair_src[k] < 0 || pair_src[k] >= c->n || pair_tgt[k] < 0 || pair_tgt[k] >= c->n) return false;
    return true;
}

// The codes of a blocking call's chunks.  Per-entry failures (missing self-loop, unreachable
// target) mark those entries only: the chunk's results are still copied out, the first such
// code is kept for the return and any other code ends the call.
struct SoftCode {
    int soft = SHD_ROUTE_OK;
    int sync(shd_route* c) {
        const int rc = shd_route_sync(c, nullptr);
        if (rc && rc != SHD_ROUTE_ENOEDGE && rc != SHD_ROUTE_EUNREACH) return rc;
        if (rc && !soft) soft = rc;
        return SHD_ROUTE_OK;
    }
};

// rows of row_bytes per device chunk of a blocking call: up to 1 GiB
int32_t host_chunk(int32_t ns, size_t row_bytes) {
    return (int32_t)std::max<size_t>(1, std::min<size_t>(ns, (size_t)(1u << 30) / row_bytes));
}

// A blocking block call: sources and targets to the device, then per chunk of sources
// launch(i0, k, d_src, d_tgt) for sources i0 .. i0 + k (d_src their first) on the null stream, the
// sync, and take(i0, k) for the chunk's results.
template <typename Launch, typename Take>
int host_blocks(shd_route* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, int32_t chunk,
                Launch launch, Take take) {
    DevBuf dsrc, dtgt;
    int rc;
    if ((rc = dsrc.alloc(sizeof(int32_t) * ns)) || (rc = dtgt.alloc(sizeof(int32_t) * std::max(nt, 1)))) return rc;
    if (hipMemcpy(dsrc.p, src, sizeof(int32_t) * ns, hipMemcpyHostToDevice) != hipSuccess ||
        (nt && hipMemcpy(dtgt.p, tgt, sizeof(int32_t) * nt, hipMemcpyHostToDevice) != hipSuccess))
        return SHD_ROUTE_EDEVICE;
    SoftCode sc;
    for (int32_t i0 = 0; i0 < ns; i0 += chunk) {
        const int32_t k = std::min(chunk, ns - i0);
        if ((rc = launch(i0, k, (const int32_t*)dsrc.p + i0, (const int32_t*)dtgt.p)) || (rc = sc.sync(c)) ||
            (rc = take(i0, k)))
            return rc;
    }
    return sc.soft;
}

int to_host(void* out, const void* dev, size_t bytes) {
    if (!out || !bytes) return SHD_ROUTE_OK;
    return hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess ? SHD_ROUTE_OK : SHD_ROUTE_EDEVICE;
}

// ---- the arcs on the device ----
// the in-CSR with edge ids and each vertex's self-loop edge (path_in_csr)
int ensure_hops(shd_route* c) {
    PathDev& p = c->path;
    if (p.hp_ready) return SHD_ROUTE_OK;
    const int n = c->n;
    const PathArcs arcs(n, c->directed, c->e_src, c->e_dst);
    const PathCsr in = path_in_csr(n, arcs, c->e_lat.data(), c->e_rel);
    std::vector<int> ident(n), z(1, 0);
    std::iota(ident.begin(), ident.end(), 0);
    int rc = upload(c, &p.hp_row, in.row);
    if (!rc) rc = upload(c, &p.hp_col, in.col);
    if (!rc) rc = upload(c, &p.hp_eid, in.eid);
    if (!rc) rc = upload(c, &p.hp_w, in.w);
    if (!rc) rc = upload(c, &p.hp_self, arcs.self);
    if (!rc) rc = upload(c, &p.hp_ident, ident);
    if (!rc) rc = upload(c, &p.hp_saved, z);
    if (!rc && n <= 65535 && kHpSmall + hp_state_bytes<uint16_t>(n) <= kLdsBudget)
        rc = hip_check(hipFuncSetAttribute((const void*)hops_depth_kernel<uint16_t, true, 1024>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(kHpSmall + hp_state_bytes<uint16_t>(n))));
    if (rc) return rc;
    p.hp_ready = 1;
    return SHD_ROUTE_OK;
}

// and for the ties the reliabilities of those in-arcs, in their order, and the out-CSR (path_out_csr)
int ensure_ties(shd_route* c) {
    PathDev& p = c->path;
    if (p.ti_ready) return SHD_ROUTE_OK;
    int rc = ensure_hops(c);
    if (rc) return rc;
    const int n = c->n;
    const PathArcs arcs(n, c->directed, c->e_src, c->e_dst);
    const PathCsr in = path_in_csr(n, arcs, c->e_lat.data(), c->e_rel);
    const PathCsr out = path_out_csr(n, arcs, c->e_lat.data(), c->e_rel);
    rc = upload(c, &p.ti_r, in.r);
    if (!rc) rc = upload(c, &p.ti_row, out.row);
    if (!rc) rc = upload(c, &p.ti_head, out.col);
    if (!rc) rc = upload(c, &p.ti_w, out.w);
    if (!rc && ties_fits_lds(n))
        rc = hip_check(hipFuncSetAttribute((const void*)ties_dag_kernel<uint16_t, true, 1024>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(kTiSmall + TiesLayout<uint16_t>::make(n).total)));
    if (rc) return rc;
    p.ti_ready = 1;
    return SHD_ROUTE_OK;
}

// and for the ECMP loads the edge id of every arc of that out-CSR, in its order
int ensure_ecmp(shd_route* c) {
    PathDev& p = c->path;
    if (p.ec_ready) return SHD_ROUTE_OK;
    int rc = ensure_ties(c);
    if (rc) return rc;
    const int n = c->n;
    const PathArcs arcs(n, c->directed, c->e_src, c->e_dst);
    const PathCsr out = path_out_csr(n, arcs, c->e_lat.data(), c->e_rel);
    rc = upload(c, &p.ec_eid, out.eid);
    if (!rc && ecmp_fits_lds(n))
        rc = hip_check(hipFuncSetAttribute((const void*)ecmp_dag_kernel<uint16_t, true, 1024>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(kEcSmall + EcmpLayout<uint16_t>::make(n).total)));
    if (rc) return rc;
    p.ec_ready = 1;
    return SHD_ROUTE_OK;
}

DevHops dev_hops(const shd_route* c) {
    const PathDev& p = c->path;
    DevHops g;
    g.n = c->n; g.row_in = p.hp_row; g.col_in = p.hp_col; g.eid_in = p.hp_eid; g.w_in = p.hp_w;
    g.self_eid = p.hp_self;
    return g;
}

DevTies dev_ties(const shd_route* c) {
    const PathDev& p = c->path;
    DevTies q;
    q.r_in = p.ti_r; q.row_out = p.ti_row; q.head_out = p.ti_head; q.w_out = p.ti_w;
    q.vf = c->d_vf; q.self_r = c->d_self_r;
    return q;
}

// the buffers grown on demand (shd_route_destroy; the uploads are in the context's allocs)
void path_free(PathDev& p) {
    for (char* q : {p.hp_ws.p, p.ld_ws.p, p.ti_ws.p, p.ec_ws.p, p.fo_ws.p, p.lo_ws.p, p.ou_ws.p, p.rp_ws.p, p.ed_ws.p, p.buf})
        if (q) (void)hipFree(q);
}

int hp_mode(const shd_route* c, uint32_t flags) {
    if (!(flags & SHD_ROUTE_DISPATCH)) return 0;
    return c->complete ? 2 : c->prefer_direct ? 1 : 0;
}

// ---- source chunks over the row scratch ----
// scratch budget of the path calls' distance, parent and hop rows (bytes)
size_t hp_budget() {
    if (const char* e = getenv("SHD_ROUTE_HOPS_SCRATCH")) {
        const unsigned long long b = strtoull(e, nullptr, 10);
        if (b > 0) return (size_t)b;
    }
    return (size_t)1 << 30;
}

// The ns sources of a call, as many at a time as the scratch budget holds (scratch_chunks):
// body(i0, k, dist, par, hrow) runs sources i0 .. i0 + k over the planes of the scratch.  Under
// dispatch on a complete graph (mode 2) nothing needs rows: one chunk of all sources, no scratch.
template <typename Body>
int source_chunks(shd_route* c, int ns, int mode, bool want_hrow, Body body) {
    if (mode == 2) return body(0, ns, (double*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr);
    PathDev& p = c->path;
    const ScratchChunks s = scratch_chunks(c->n, ns, hp_budget(), want_hrow);
    if (s.bytes > p.buf_cap) {
        if (p.buf) (void)hipFree(p.buf);
        p.buf = nullptr;
        p.buf_cap = 0;
        if (hipMalloc((void**)&p.buf, s.bytes) != hipSuccess) return SHD_ROUTE_ENOMEM;
        p.buf_cap = s.bytes;
    }
    for (int i0 = 0; i0 < ns; i0 += s.chunk)
        if (int rc = body(i0, std::min(s.chunk, ns - i0), (double*)p.buf, (uint32_t*)(p.buf + s.par_off),
                          want_hrow ? (int32_t*)(p.buf + s.hrow_off) : nullptr))
            return rc;
    return SHD_ROUTE_OK;
}

// dist (k x n f64) = the all-vertex latency rows of the sources.  The rows raise no code of
// their own here (a source without a self-loop is the caller's to judge): the error word is
// parked around them.
int all_vertex_rows(shd_route* c, const int32_t* d_src, int k, double* dist, hipStream_t st) {
    const PathDev& p = c->path;
    hipLaunchKernelGGL(hops_err_park_kernel, dim3(1), dim3(1), 0, st, c->d_err, p.hp_saved);
    const int rc = shd_route_rows_async(c, d_src, k, p.hp_ident, c->n, c->n, 0u, dist, nullptr, nullptr, st);
    hipLaunchKernelGGL(hops_err_unpark_kernel, dim3(1), dim3(1), 0, st, c->d_err, (const int*)p.hp_saved);
    return rc;
}

dim3 per_vertex_grid(const shd_route* c, int k) {
    return dim3((unsigned)std::min((c->n + 255) / 256, 4096), (unsigned)std::min(k, 65535));
}

// ---- the per-source state kernels ----
// A kernel family K<T, kLds, 1024> in the form f (state_form): launch(tag, ws, stride) spells
// the family's one hipLaunchKernelGGL with T = tag.t and kLds = tag.lds.  The HBM forms take
// their slices from `slices`, regrown when the launch needs more than they hold.
template <typename T, bool kLds>
struct StateTag {
    using t = T;
    static constexpr bool lds = kLds;
};

template <typename Launch>
int launch_state(PathSlices& slices, const StateLaunch& f, hipStream_t st, Launch launch) {
    if (f.form >= kStateHbm16 && f.stride * (size_t)f.grid > slices.cap) {
        // a launch of this context that still uses the old slices is on the same stream or
        // synchronised (one rows launch at a time): wait before the slices go
        if (slices.p) {
            if (hipStreamSynchronize(st) != hipSuccess) return SHD_ROUTE_EDEVICE;
            (void)hipFree(slices.p);
        }
        slices.p = nullptr;
        slices.cap = 0;
        if (hipMalloc((void**)&slices.p, f.stride * (size_t)f.slots) != hipSuccess) return SHD_ROUTE_ENOMEM;
        slices.cap = f.stride * (size_t)f.slots;
    }
    switch (f.form) {
        case kStateLds: launch(StateTag<uint16_t, true>{}, (char*)nullptr, (size_t)0); break;
        case kStateHbm16: launch(StateTag<uint16_t, false>{}, slices.p, f.stride); break;
        case kStateHbm32: launch(StateTag<uint32_t, false>{}, slices.p, f.stride); break;
        default: launch(StateTag<uint16_t, false>{}, (char*)nullptr, (size_t)0); break;
    }
    return hip_check(hipGetLastError());
}

// ---- hops ----
// the hop rows of k sources from their parent rows (hops_depth_kernel).  The HBM slices take
// 256 MiB at the most, so they are sized by the first launch and never regrown.
int hp_depth(shd_route* c, const uint32_t* par, const int32_t* d_src, int k, const int32_t* d_tgt, int nt,
             long long ld, int mode, int quiet, int32_t* d_hops, int32_t* d_row_max, hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    const char* e = getenv("SHD_ROUTE_HOPS_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, mode, k, kHpSmall, hp_state_bytes<uint16_t>(n), kLdsBudget, knob_off(e),
                                     a16(hp_state_bytes<uint16_t>(n)), a16(hp_state_bytes<uint32_t>(n)),
                                     (size_t)256 << 20);
    return launch_state(c->path.hp_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((hops_depth_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g,
                           par, (long long)n, d_src, k, d_tgt, nt, ld, mode, quiet, d_hops, d_row_max, ws, stride,
                           c->d_err);
    });
}

// the trees of k sources: dist = their all-vertex latency rows, par (k x n u32) the parent arc
// of every vertex and, where hrow is given, its hop count (k x n i32, -1 without a raise)
int hp_trees(shd_route* c, const int32_t* d_src, int k, double* dist, uint32_t* par, int32_t* hrow, hipStream_t st) {
    const int n = c->n;
    int rc = all_vertex_rows(c, d_src, k, dist, st);
    if (rc) return rc;
    hipLaunchKernelGGL(hops_parent_kernel<256>, per_vertex_grid(c, k), dim3(256), 0, st, dev_hops(c),
                       (const double*)dist, (long long)n, d_src, k, par, (long long)n, c->d_err);
    if ((rc = hip_check(hipGetLastError())) || !hrow) return rc;
    return hp_depth(c, par, d_src, k, c->path.hp_ident, n, (long long)n, 0, 1, hrow, nullptr, st);
}

}  // namespace

extern "C" {

int shd_route_hops_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                         int64_t ld, uint32_t flags, int32_t* d_hops, int32_t* d_row_max, void* stream) {
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld)) return SHD_ROUTE_EINVAL;
    if (ns == 0) return SHD_ROUTE_OK;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    int rc = ensure_hops(c);
    if (rc) return rc;
    const int mode = hp_mode(c, flags);
    return source_chunks(c, ns, mode, false, [&](int i0, int k, double* dist, uint32_t* par, int32_t*) {
        if (par && (rc = hp_trees(c, d_src + i0, k, dist, par, nullptr, st))) return rc;
        return hp_depth(c, par, d_src + i0, k, d_tgt, nt, (long long)ld, mode, 0,
                        d_hops ? d_hops + (long long)i0 * ld : nullptr, d_row_max ? d_row_max + i0 : nullptr, st);
    });
}

int shd_route_hops(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, uint32_t flags,
                   int32_t* hops_out, int32_t* row_max_out) {
    if (!block_args_ok(c, src, ns, tgt, nt, nt)) return SHD_ROUTE_EINVAL;
    if (ns == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const size_t row_bytes = sizeof(int32_t) * (size_t)std::max(nt, 1);
    const int32_t chunk = host_chunk(ns, row_bytes);
    DevBuf dh, dm;
    int rc;
    if ((rc = dh.alloc(row_bytes * chunk)) || (rc = dm.alloc(sizeof(int32_t) * chunk))) return rc;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            return shd_route_hops_async(c, d_src, k, d_tgt, nt, nt, flags, (int32_t*)dh.p, (int32_t*)dm.p, nullptr);
        },
        [&](int32_t i0, int32_t k) {
            if (int r = to_host(hops_out ? hops_out + (size_t)i0 * nt : nullptr, dh.p, sizeof(int32_t) * (size_t)nt * k))
                return r;
            return to_host(row_max_out ? row_max_out + i0 : nullptr, dm.p, sizeof(int32_t) * k);
        });
}

int shd_route_paths(shd_route_t* c, const int32_t* pair_src, const int32_t* pair_tgt, int64_t npairs, uint32_t flags,
                    int64_t* off_out, int32_t* vert_out, int32_t* edge_out, int64_t cap) {
    if (!pair_args_ok(c, pair_src, pair_tgt, npairs) || !off_out || cap < 0 || (cap > 0 && (!vert_out || !edge_out)))
        return SHD_ROUTE_EINVAL;
    off_out[0] = 0;
    if (npairs == 0) return SHD_ROUTE_OK;
    const int n = c->n;
    const int np = (int)npairs;
    if (!pairs_in_range(c, pair_src, pair_tgt, np)) return SHD_ROUTE_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    int rc = ensure_hops(c);
    if (rc) return rc;
    const int mode = hp_mode(c, flags);
    const bool want = vert_out != nullptr && cap > 0;
    const PairGroups pg = group_pairs(pair_src, pair_tgt, nullptr, np);
    std::vector<int32_t> gcnt(np, -1);       // hop count of each grouped pair
    std::vector<int64_t> gvo(np, 0), geo(np, 0);  // its place in the staged vertices / edges
    std::vector<int32_t> sv, se;             // paths staged in grouped order
    SoftCode sc;
    const DevHops g = dev_hops(c);
    // the distinct sources in chunks: distance, parent and hop rows within the scratch budget
    rc = source_chunks(c, (int)pg.us.size(), mode, true, [&](int u0, int k, double* dist, uint32_t* par, int32_t* hrow) {
        const int g0 = (int)pg.first[u0], cp = (int)pg.first[u0 + k] - g0;
        DevBuf dsrc, dsi, dtg, dcnt;
        if ((rc = dsrc.alloc(sizeof(int32_t) * k)) || (rc = dsi.alloc(sizeof(int32_t) * cp)) ||
            (rc = dtg.alloc(sizeof(int32_t) * cp)) || (rc = dcnt.alloc(sizeof(int32_t) * cp)))
            return rc;
        std::vector<int32_t> lsi(cp);
        for (int q = 0; q < cp; q++) lsi[q] = pg.gsi[g0 + q] - u0;
        if (hipMemcpy(dsrc.p, pg.us.data() + u0, sizeof(int32_t) * k, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dsi.p, lsi.data(), sizeof(int32_t) * cp, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dtg.p, pg.gt.data() + g0, sizeof(int32_t) * cp, hipMemcpyHostToDevice) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        if (par && (rc = hp_trees(c, (const int32_t*)dsrc.p, k, dist, par, hrow, nullptr))) return rc;
        const int pgrid = std::min((cp + 255) / 256, 4096);
        hipLaunchKernelGGL(hops_pairs_kernel, dim3(pgrid), dim3(256), 0, nullptr, g, (const int*)dsrc.p,
                           (const int*)dsi.p, (const int*)dtg.p, cp, mode, (const int*)hrow, (int*)dcnt.p, c->d_err);
        if ((rc = hip_check(hipGetLastError())) || (rc = sc.sync(c))) return rc;
        if (hipMemcpy(gcnt.data() + g0, dcnt.p, sizeof(int32_t) * cp, hipMemcpyDeviceToHost) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        if (!want) return SHD_ROUTE_OK;
        // this chunk's paths, packed in grouped order behind the chunks before it
        std::vector<long long> lvo(cp), leo(cp);
        long long tv = 0, te = 0;
        for (int q = 0; q < cp; q++) {
            lvo[q] = tv; leo[q] = te;
            gvo[g0 + q] = (int64_t)sv.size() + tv;
            geo[g0 + q] = (int64_t)se.size() + te;
            if (gcnt[g0 + q] >= 0) { tv += gcnt[g0 + q] + 1; te += gcnt[g0 + q]; }
        }
        if (tv == 0) return SHD_ROUTE_OK;
        DevBuf dvo, deo, dv, de;
        if ((rc = dvo.alloc(sizeof(long long) * cp)) || (rc = deo.alloc(sizeof(long long) * cp)) ||
            (rc = dv.alloc(sizeof(int32_t) * (size_t)tv)) || (rc = de.alloc(sizeof(int32_t) * (size_t)std::max(te, 1LL))))
            return rc;
        if (hipMemcpy(dvo.p, lvo.data(), sizeof(long long) * cp, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(deo.p, leo.data(), sizeof(long long) * cp, hipMemcpyHostToDevice) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        hipLaunchKernelGGL(hops_extract_kernel, dim3(pgrid), dim3(256), 0, nullptr, g, (const uint32_t*)par,
                           (long long)n, (const int*)dsrc.p, (const int*)dsi.p, (const int*)dtg.p, (const int*)dcnt.p,
                           (const long long*)dvo.p, (const long long*)deo.p, cp, mode, (int*)dv.p, (int*)de.p, c->d_err);
        if ((rc = hip_check(hipGetLastError())) || (rc = shd_route_sync(c, nullptr))) return rc;
        const size_t v0 = sv.size(), e0 = se.size();
        sv.resize(v0 + (size_t)tv);
        se.resize(e0 + (size_t)te);
        if ((rc = to_host(sv.data() + v0, dv.p, sizeof(int32_t) * (size_t)tv))) return rc;
        return to_host(se.data() + e0, de.p, sizeof(int32_t) * (size_t)te);
    });
    if (rc) return rc;
    // offsets in the caller's pair order; a failed pair takes no room
    std::vector<int> gpos(np);
    for (int gq = 0; gq < np; gq++) gpos[pg.order[gq]] = gq;
    for (int k = 0; k < np; k++) {
        const int32_t h = gcnt[gpos[k]];
        off_out[k + 1] = off_out[k] + (h >= 0 ? h + 1 : 0);
    }
    if (off_out[np] > cap) return SHD_ROUTE_EINVAL;
    int64_t done = 0;  // pairs before k that did not fail: their edges take one slot less each
    for (int k = 0; k < np; k++) {
        const int gq = gpos[k];
        const int32_t h = gcnt[gq];
        if (h < 0) continue;
        std::memcpy(vert_out + off_out[k], sv.data() + gvo[gq], sizeof(int32_t) * (size_t)(h + 1));
        std::memcpy(edge_out + (off_out[k] - done), se.data() + geo[gq], sizeof(int32_t) * (size_t)h);
        done++;
    }
    return sc.soft;
}

}  // extern "C"

// ---- link loads ----
namespace {

// the tree sums of k sources (loads_tree_kernel); the HBM slices take a quarter of the scratch budget
int ld_tree(shd_route* c, const uint32_t* par, const int32_t* hrow, const int32_t* d_src, int k,
            const int32_t* d_tgt, int nt, long long ld, const long long* d_eoff, const uint64_t* d_wt, int mode,
            uint64_t* d_edge, uint64_t* d_transit, uint64_t* d_unrouted, hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    if (mode != 2 && !c->path.ld_ready && n <= 65535 && kLdSmall + ld_state_bytes<uint16_t>(n) <= kLdsBudget) {
        int rc = hip_check(hipFuncSetAttribute((const void*)loads_tree_kernel<uint16_t, true, 1024>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        if (rc) return rc;
        c->path.ld_ready = 1;
    }
    const char* e = getenv("SHD_ROUTE_LOADS_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, mode, k, kLdSmall, ld_state_bytes<uint16_t>(n), kLdsBudget, knob_off(e),
                                     a16(ld_state_bytes<uint16_t>(n)), a16(ld_state_bytes<uint32_t>(n)),
                                     hp_budget() / 4);
    return launch_state(c->path.ld_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((loads_tree_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g,
                           par, hrow, d_src, k, d_tgt, nt, ld, d_eoff, (const unsigned long long*)d_wt, mode,
                           (unsigned long long*)d_edge, (unsigned long long*)d_transit,
                           (unsigned long long*)d_unrouted, ws, stride, c->d_err);
    });
}

// The loads of ns sources added into the outputs.  Entries: the block (d_eoff null: d_tgt[nt],
// d_wt row stride ld) or the sparse lists d_eoff gives, whose positions into d_tgt / d_wt are
// absolute: a later chunk advances d_eoff alone.
int ld_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, long long ld,
               const long long* d_eoff, const uint64_t* d_wt, uint32_t flags, uint64_t* d_edge, uint64_t* d_transit,
               uint64_t* d_unrouted, hipStream_t st) {
    int rc = ensure_hops(c);
    if (rc) return rc;
    const int mode = hp_mode(c, flags);
    return source_chunks(c, ns, mode, true, [&](int i0, int k, double* dist, uint32_t* par, int32_t* hrow) {
        if (par && (rc = hp_trees(c, d_src + i0, k, dist, par, hrow, st))) return rc;
        return ld_tree(c, par, hrow, d_src + i0, k, d_tgt, nt, ld, d_eoff ? d_eoff + i0 : nullptr,
                       d_wt && !d_eoff ? d_wt + (long long)i0 * ld : d_wt, mode, d_edge, d_transit, d_unrouted, st);
    });
}

// zero the outputs a call without SHD_ROUTE_LOADS_ADD starts from
int ld_zero(shd_route* c, uint32_t flags, uint64_t* d_edge, uint64_t* d_transit, uint64_t* d_unrouted, hipStream_t st) {
    if (flags & SHD_ROUTE_LOADS_ADD) return SHD_ROUTE_OK;
    if ((d_edge && c->m && hipMemsetAsync(d_edge, 0, sizeof(uint64_t) * (size_t)c->m, st) != hipSuccess) ||
        (d_transit && hipMemsetAsync(d_transit, 0, sizeof(uint64_t) * (size_t)c->n, st) != hipSuccess) ||
        (d_unrouted && hipMemsetAsync(d_unrouted, 0, sizeof(uint64_t), st) != hipSuccess))
        return SHD_ROUTE_EDEVICE;
    return SHD_ROUTE_OK;
}

// device accumulators of the blocking calls: zeroed, summed into by every chunk, then copied
// (or, with SHD_ROUTE_LOADS_ADD, added) into the caller's host arrays
struct LoadsOut {
    DevBuf de, dt, du;
    int m = 0, n = 0;
    int init(const shd_route* c) {
        m = c->m; n = c->n;
        int rc;
        if ((rc = de.alloc(sizeof(uint64_t) * (size_t)m)) || (rc = dt.alloc(sizeof(uint64_t) * (size_t)n)) ||
            (rc = du.alloc(sizeof(uint64_t))))
            return rc;
        if ((m && hipMemset(de.p, 0, sizeof(uint64_t) * (size_t)m) != hipSuccess) ||
            hipMemset(dt.p, 0, sizeof(uint64_t) * (size_t)n) != hipSuccess ||
            hipMemset(du.p, 0, sizeof(uint64_t)) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        return SHD_ROUTE_OK;
    }
    static int take(uint64_t* out, const void* dev, size_t count, bool add) {
        if (!add) return to_host(out, dev, sizeof(uint64_t) * count);
        if (!out || !count) return SHD_ROUTE_OK;
        std::vector<uint64_t> h(count);
        if (int rc = to_host(h.data(), dev, sizeof(uint64_t) * count)) return rc;
        for (size_t q = 0; q < count; q++) out[q] += h[q];
        return SHD_ROUTE_OK;
    }
    int finish(uint32_t flags, uint64_t* edge_out, uint64_t* transit_out, uint64_t* unrouted_out) {
        const bool add = (flags & SHD_ROUTE_LOADS_ADD) != 0;
        int rc;
        if ((rc = take(edge_out, de.p, (size_t)m, add)) || (rc = take(transit_out, dt.p, (size_t)n, add))) return rc;
        return take(unrouted_out, du.p, 1, add);
    }
    // ns sources on the null stream into the accumulators
    int add_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, const long long* d_eoff,
                    const void* d_wt, uint32_t flags) {
        return ld_sources(c, d_src, ns, d_tgt, nt, nt, d_eoff, (const uint64_t*)d_wt, flags, (uint64_t*)de.p,
                          (uint64_t*)dt.p, (uint64_t*)du.p, nullptr);
    }
};

// the outputs of a blocking call that has nothing to route
void ld_host_zero(const shd_route* c, uint32_t flags, uint64_t* edge_out, uint64_t* transit_out, uint64_t* unrouted_out) {
    if (flags & SHD_ROUTE_LOADS_ADD) return;
    if (edge_out) std::fill(edge_out, edge_out + c->m, (uint64_t)0);
    if (transit_out) std::fill(transit_out, transit_out + c->n, (uint64_t)0);
    if (unrouted_out) *unrouted_out = 0;
}

}  // namespace

extern "C" {

int shd_route_loads_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                          int64_t ld, uint32_t flags, const uint64_t* d_wt, uint64_t* d_edge_load, uint64_t* d_transit,
                          uint64_t* d_unrouted, void* stream) {
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld)) return SHD_ROUTE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    int rc = ld_zero(c, flags, d_edge_load, d_transit, d_unrouted, st);
    if (rc || ns == 0 || nt == 0) return rc;
    return ld_sources(c, d_src, ns, d_tgt, nt, (long long)ld, nullptr, d_wt, flags, d_edge_load, d_transit, d_unrouted,
                      st);
}

int shd_route_loads(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, uint32_t flags,
                    const uint64_t* wt, uint64_t* edge_load_out, uint64_t* transit_out, uint64_t* unrouted_out) {
    if (!block_args_ok(c, src, ns, tgt, nt, nt)) return SHD_ROUTE_EINVAL;
    for (int32_t i = 0; i < ns; i++)
        if (src[i] < 0 || src[i] >= c->n) return SHD_ROUTE_EINVAL;
    for (int32_t j = 0; j < nt; j++)
        if (tgt[j] < 0 || tgt[j] >= c->n) return SHD_ROUTE_EINVAL;
    if (ns == 0 || nt == 0) {
        ld_host_zero(c, flags, edge_load_out, transit_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const size_t row_bytes = sizeof(uint64_t) * (size_t)nt;
    const int32_t chunk = host_chunk(ns, row_bytes);
    DevBuf dw;
    LoadsOut out;
    int rc;
    if ((wt && (rc = dw.alloc(row_bytes * chunk))) || (rc = out.init(c))) return rc;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t i0, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            if (wt && hipMemcpy(dw.p, wt + (size_t)i0 * nt, row_bytes * k, hipMemcpyHostToDevice) != hipSuccess)
                return SHD_ROUTE_EDEVICE;
            return out.add_sources(c, d_src, k, d_tgt, nt, nullptr, wt ? dw.p : nullptr, flags);
        },
        [&](int32_t i0, int32_t k) {
            return i0 + k < ns ? SHD_ROUTE_OK : out.finish(flags, edge_load_out, transit_out, unrouted_out);
        });
}

int shd_route_pair_loads(shd_route_t* c, const int32_t* pair_src, const int32_t* pair_tgt, const uint64_t* pair_wt,
                         int64_t npairs, uint32_t flags, uint64_t* edge_load_out, uint64_t* transit_out,
                         uint64_t* unrouted_out) {
    if (!pair_args_ok(c, pair_src, pair_tgt, npairs) || !pairs_in_range(c, pair_src, pair_tgt, (int)npairs))
        return SHD_ROUTE_EINVAL;
    const int np = (int)npairs;
    if (np == 0) {
        ld_host_zero(c, flags, edge_load_out, transit_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    // the entries of distinct source u are the grouped positions first[u] .. first[u + 1]
    const PairGroups pg = group_pairs(pair_src, pair_tgt, pair_wt, np);
    const int nu = (int)pg.us.size();
    DevBuf dsrc, dtgt, dw, doff;
    LoadsOut out;
    int rc;
    if ((rc = dsrc.alloc(sizeof(int32_t) * nu)) || (rc = dtgt.alloc(sizeof(int32_t) * (size_t)np)) ||
        (pair_wt && (rc = dw.alloc(sizeof(uint64_t) * (size_t)np))) ||
        (rc = doff.alloc(sizeof(long long) * ((size_t)nu + 1))) || (rc = out.init(c)))
        return rc;
    if (hipMemcpy(dsrc.p, pg.us.data(), sizeof(int32_t) * nu, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dtgt.p, pg.gt.data(), sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess ||
        (pair_wt && hipMemcpy(dw.p, pg.gw.data(), sizeof(uint64_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(doff.p, pg.first.data(), sizeof(long long) * ((size_t)nu + 1), hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    SoftCode sc;
    if ((rc = out.add_sources(c, (const int32_t*)dsrc.p, nu, (const int32_t*)dtgt.p, 0, (const long long*)doff.p,
                              pair_wt ? dw.p : nullptr, flags)) ||
        (rc = sc.sync(c)) || (rc = out.finish(flags, edge_load_out, transit_out, unrouted_out)))
        return rc;
    return sc.soft;
}

}  // extern "C"

// ---- path folds ----
namespace {

// the ops of a call, by value for the kernel
bool fold_ops_ok(const int32_t* ops, int32_t nf, FoldOps* out) {
    if (!ops || nf < 1 || nf > SHD_ROUTE_FOLD_MAX_N) return false;
    for (int k = 0; k < SHD_ROUTE_FOLD_MAX_N; k++) out->op[k] = SHD_ROUTE_FOLD_SUM;
    for (int k = 0; k < nf; k++) {
        if (ops[k] < SHD_ROUTE_FOLD_SUM || ops[k] > SHD_ROUTE_FOLD_PROD) return false;
        out->op[k] = ops[k];
    }
    return true;
}

bool fold_has_nan(const double* val, size_t count) {
    for (size_t q = 0; q < count; q++)
        if (val[q] != val[q]) return true;
    return false;
}

// the sweeps of k sources and their entries (fold_tree_kernel); HBM slices within 256 MiB, regrown
// as the loads'
int fo_tree(shd_route* c, const uint32_t* par, const int32_t* hrow, const int32_t* d_src, int k, const int32_t* d_tgt,
            int nt, long long ld, const long long* d_eoff, const FoldOps& ops, int nf, const double* d_val, int mode,
            double* d_out, long long plane, hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    if (mode != 2 && !c->path.fo_ready && fold_fits_lds(n)) {
        int rc = hip_check(hipFuncSetAttribute((const void*)fold_tree_kernel<uint16_t, true, 1024>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFoldLdsBudget));
        if (rc) return rc;
        c->path.fo_ready = 1;
    }
    const char* e = getenv("SHD_ROUTE_FOLD_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, mode, k, kFoSmall, FoldLayout<uint16_t>::make(n).total, kFoldLdsBudget,
                                     knob_off(e), a16(FoldLayout<uint16_t>::make(n).total),
                                     a16(FoldLayout<uint32_t>::make(n).total), (size_t)256 << 20);
    return launch_state(c->path.fo_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((fold_tree_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g,
                           par, hrow, d_src, k, d_tgt, nt, ld, d_eoff, ops, nf, d_val, (long long)c->m, mode, d_out,
                           plane, ws, stride, c->d_err);
    });
}

// The nf folds of ns sources.  Entries as ld_sources takes them: the block, whose chunk i0
// writes from row i0 of every plane on, or the sparse lists of d_eoff with absolute positions.
int fo_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, long long ld,
               const long long* d_eoff, const FoldOps& ops, int nf, const double* d_val, uint32_t flags, double* d_out,
               long long plane, hipStream_t st) {
    int rc = ensure_hops(c);
    if (rc) return rc;
    const int mode = hp_mode(c, flags);
    return source_chunks(c, ns, mode, true, [&](int i0, int k, double* dist, uint32_t* par, int32_t* hrow) {
        if (par && (rc = hp_trees(c, d_src + i0, k, dist, par, hrow, st))) return rc;
        return fo_tree(c, par, hrow, d_src + i0, k, d_tgt, nt, ld, d_eoff ? d_eoff + i0 : nullptr, ops, nf, d_val, mode,
                       d_eoff ? d_out : d_out + (long long)i0 * ld, plane, st);
    });
}

}  // namespace

extern "C" {

int shd_route_fold_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                         int64_t ld, uint32_t flags, const int32_t* ops, int32_t nf, const double* d_val,
                         double* d_out, int64_t plane, void* stream) {
    FoldOps fo;
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld) || !fold_ops_ok(ops, nf, &fo) || !d_val ||
        plane < (int64_t)ns * ld || (ns && nt && !d_out))
        return SHD_ROUTE_EINVAL;
    if (ns == 0 || nt == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    return fo_sources(c, d_src, ns, d_tgt, nt, (long long)ld, nullptr, fo, nf, d_val, flags, d_out, (long long)plane,
                      (hipStream_t)stream);
}

int shd_route_fold(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, uint32_t flags,
                   const int32_t* ops, int32_t nf, const double* val, double* out) {
    FoldOps fo;
    if (!block_args_ok(c, src, ns, tgt, nt, nt) || !fold_ops_ok(ops, nf, &fo) || !val || (ns && nt && !out))
        return SHD_ROUTE_EINVAL;
    for (int32_t i = 0; i < ns; i++)
        if (src[i] < 0 || src[i] >= c->n) return SHD_ROUTE_EINVAL;
    for (int32_t j = 0; j < nt; j++)
        if (tgt[j] < 0 || tgt[j] >= c->n) return SHD_ROUTE_EINVAL;
    const size_t vals = (size_t)nf * (size_t)c->m;
    if (fold_has_nan(val, vals)) return SHD_ROUTE_EINVAL;
    if (ns == 0 || nt == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const size_t row_bytes = sizeof(double) * (size_t)nt;
    const int32_t chunk = host_chunk(ns, row_bytes * nf);
    const size_t dplane = (size_t)chunk * nt;  // one fold of a chunk on the device
    DevBuf dv, dout;
    int rc;
    if ((rc = dv.alloc(sizeof(double) * vals)) || (rc = dout.alloc(sizeof(double) * dplane * nf))) return rc;
    if (vals && hipMemcpy(dv.p, val, sizeof(double) * vals, hipMemcpyHostToDevice) != hipSuccess) return SHD_ROUTE_EDEVICE;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            return shd_route_fold_async(c, d_src, k, d_tgt, nt, nt, flags, ops, nf, (const double*)dv.p, (double*)dout.p,
                                        (int64_t)dplane, nullptr);
        },
        [&](int32_t i0, int32_t k) {
            for (int f = 0; f < nf; f++)
                if (int r = to_host(out + (size_t)f * ns * nt + (size_t)i0 * nt, (const double*)dout.p + f * dplane,
                                    row_bytes * k))
                    return r;
            return SHD_ROUTE_OK;
        });
}

int shd_route_pair_fold(shd_route_t* c, const int32_t* pair_src, const int32_t* pair_tgt, int64_t npairs,
                        uint32_t flags, const int32_t* ops, int32_t nf, const double* val, double* out) {
    FoldOps fo;
    if (!pair_args_ok(c, pair_src, pair_tgt, npairs) || !pairs_in_range(c, pair_src, pair_tgt, (int)npairs) ||
        !fold_ops_ok(ops, nf, &fo) || !val || (npairs && !out))
        return SHD_ROUTE_EINVAL;
    const size_t vals = (size_t)nf * (size_t)c->m;
    if (fold_has_nan(val, vals)) return SHD_ROUTE_EINVAL;
    const int np = (int)npairs;
    if (np == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    // the entries of distinct source u are the grouped positions first[u] .. first[u + 1]
    const PairGroups pg = group_pairs(pair_src, pair_tgt, nullptr, np);
    const int nu = (int)pg.us.size();
    DevBuf dsrc, dtgt, doff, dv, dout;
    int rc;
    if ((rc = dsrc.alloc(sizeof(int32_t) * nu)) || (rc = dtgt.alloc(sizeof(int32_t) * (size_t)np)) ||
        (rc = doff.alloc(sizeof(long long) * ((size_t)nu + 1))) || (rc = dv.alloc(sizeof(double) * vals)) ||
        (rc = dout.alloc(sizeof(double) * (size_t)np * nf)))
        return rc;
    if (hipMemcpy(dsrc.p, pg.us.data(), sizeof(int32_t) * nu, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dtgt.p, pg.gt.data(), sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(doff.p, pg.first.data(), sizeof(long long) * ((size_t)nu + 1), hipMemcpyHostToDevice) != hipSuccess ||
        (vals && hipMemcpy(dv.p, val, sizeof(double) * vals, hipMemcpyHostToDevice) != hipSuccess))
        return SHD_ROUTE_EDEVICE;
    SoftCode sc;
    std::vector<double> grouped((size_t)np * nf);
    if ((rc = fo_sources(c, (const int32_t*)dsrc.p, nu, (const int32_t*)dtgt.p, 0, 0, (const long long*)doff.p, fo, nf,
                         (const double*)dv.p, flags, (double*)dout.p, (long long)np, nullptr)) ||
        (rc = sc.sync(c)) || (rc = to_host(grouped.data(), dout.p, sizeof(double) * grouped.size())))
        return rc;
    // back to the caller's pair order
    for (int f = 0; f < nf; f++)
        for (int gq = 0; gq < np; gq++) out[(size_t)f * np + pg.order[gq]] = grouped[(size_t)f * np + gq];
    return sc.soft;
}

}  // extern "C"

// ---- tie envelope ----
namespace {

// the sweep of k sources and their entries (ties_dag_kernel); HBM slices as the loads'
int ti_dag(shd_route* c, const double* dist, const uint32_t* rem, const int32_t* d_src, int k, const int32_t* d_tgt,
           int nt, long long ld, int mode, uint64_t* d_count, double* d_lo, double* d_hi, hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    const DevTies q = dev_ties(c);
    const char* e = getenv("SHD_ROUTE_TIES_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, mode, k, kTiSmall, TiesLayout<uint16_t>::make(n).total, kTiesLdsBudget,
                                     knob_off(e), a16(TiesLayout<uint16_t>::make(n).total),
                                     a16(TiesLayout<uint32_t>::make(n).total), hp_budget() / 4);
    return launch_state(c->path.ti_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((ties_dag_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g, q,
                           dist, rem, d_src, k, d_tgt, nt, ld, mode, (unsigned long long*)d_count, d_lo, d_hi, ws,
                           stride, c->d_err);
    });
}

}  // namespace

extern "C" {

int shd_route_ties_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                         int64_t ld, uint32_t flags, uint64_t* d_count, double* d_rel_lo, double* d_rel_hi,
                         void* stream) {
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld)) return SHD_ROUTE_EINVAL;
    if (ns == 0) return SHD_ROUTE_OK;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    int rc = ensure_ties(c);
    if (rc) return rc;
    const int mode = hp_mode(c, flags);
    const int n = c->n;
    // per chunk: dist = the sources' all-vertex latency rows, rem (k x n u32) the tight in-degree
    // of every vertex under each, then the sweep
    return source_chunks(c, ns, mode, false, [&](int i0, int k, double* dist, uint32_t* rem, int32_t*) {
        if (rem) {
            if ((rc = all_vertex_rows(c, d_src + i0, k, dist, st))) return rc;
            hipLaunchKernelGGL(ties_indeg_kernel<256>, per_vertex_grid(c, k), dim3(256), 0, st, dev_hops(c),
                               (const double*)dist, (long long)n, d_src + i0, k, rem, (long long)n);
            if ((rc = hip_check(hipGetLastError()))) return rc;
        }
        const long long o = (long long)i0 * ld;
        return ti_dag(c, dist, rem, d_src + i0, k, d_tgt, nt, (long long)ld, mode, d_count ? d_count + o : nullptr,
                      d_rel_lo ? d_rel_lo + o : nullptr, d_rel_hi ? d_rel_hi + o : nullptr, st);
    });
}

int shd_route_ties(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, uint32_t flags,
                   uint64_t* count_out, double* rel_lo_out, double* rel_hi_out) {
    if (!block_args_ok(c, src, ns, tgt, nt, nt)) return SHD_ROUTE_EINVAL;
    if (ns == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    // the three outputs: 24 bytes per entry
    const size_t row_elems = (size_t)std::max(nt, 1);
    const int32_t chunk = host_chunk(ns, 24 * row_elems);
    DevBuf dc, dl, dh;
    int rc;
    if ((count_out && (rc = dc.alloc(sizeof(uint64_t) * row_elems * chunk))) ||
        (rel_lo_out && (rc = dl.alloc(sizeof(double) * row_elems * chunk))) ||
        (rel_hi_out && (rc = dh.alloc(sizeof(double) * row_elems * chunk))))
        return rc;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            return shd_route_ties_async(c, d_src, k, d_tgt, nt, nt, flags, (uint64_t*)dc.p, (double*)dl.p,
                                        (double*)dh.p, nullptr);
        },
        [&](int32_t i0, int32_t k) {
            const size_t o = (size_t)i0 * nt, bytes = 8 * (size_t)nt * k;
            int r;
            if ((r = to_host(count_out ? count_out + o : nullptr, dc.p, bytes)) ||
                (r = to_host(rel_lo_out ? rel_lo_out + o : nullptr, dl.p, bytes)))
                return r;
            return to_host(rel_hi_out ? rel_hi_out + o : nullptr, dh.p, bytes);
        });
}

}  // extern "C"

// ---- ECMP link loads ----
namespace {

// the sweeps of k sources and their entries (ecmp_dag_kernel); HBM slices as the loads'
int ec_dag(shd_route* c, const double* dist, const uint32_t* rem, const int32_t* d_src, int k, const int32_t* d_tgt,
           int nt, long long ld, const long long* d_eoff, const uint64_t* d_wt, int mode, double* d_edge,
           double* d_transit, uint64_t* d_unrouted, hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    const DevTies q = dev_ties(c);
    const char* e = getenv("SHD_ROUTE_ECMP_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, mode, k, kEcSmall, EcmpLayout<uint16_t>::make(n).total, kEcmpLdsBudget,
                                     knob_off(e), a16(EcmpLayout<uint16_t>::make(n).total),
                                     a16(EcmpLayout<uint32_t>::make(n).total), hp_budget() / 4);
    return launch_state(c->path.ec_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((ecmp_dag_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g, q,
                           (const int*)c->path.ec_eid, dist, rem, d_src, k, d_tgt, nt, ld, d_eoff,
                           (const unsigned long long*)d_wt, mode, d_edge, d_transit, (unsigned long long*)d_unrouted,
                           ws, stride, c->d_err);
    });
}

// The ECMP loads of ns sources added into the outputs; entries as ld_sources takes them.  Per
// chunk, as shd_route_ties_async: the sources' all-vertex latency rows, the tight in-degree of
// every vertex under each, then the sweeps.
int ec_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, long long ld,
               const long long* d_eoff, const uint64_t* d_wt, uint32_t flags, double* d_edge, double* d_transit,
               uint64_t* d_unrouted, hipStream_t st) {
    int rc = ensure_ecmp(c);
    if (rc) return rc;
    const int mode = hp_mode(c, flags);
    const int n = c->n;
    return source_chunks(c, ns, mode, false, [&](int i0, int k, double* dist, uint32_t* rem, int32_t*) {
        if (rem) {
            if ((rc = all_vertex_rows(c, d_src + i0, k, dist, st))) return rc;
            hipLaunchKernelGGL(ties_indeg_kernel<256>, per_vertex_grid(c, k), dim3(256), 0, st, dev_hops(c),
                               (const double*)dist, (long long)n, d_src + i0, k, rem, (long long)n);
            if ((rc = hip_check(hipGetLastError()))) return rc;
        }
        return ec_dag(c, dist, rem, d_src + i0, k, d_tgt, nt, ld, d_eoff ? d_eoff + i0 : nullptr,
                      d_wt && !d_eoff ? d_wt + (long long)i0 * ld : d_wt, mode, d_edge, d_transit, d_unrouted, st);
    });
}

// zero the outputs a call without SHD_ROUTE_LOADS_ADD starts from (0.0 is all bits zero)
int ec_zero(shd_route* c, uint32_t flags, double* d_edge, double* d_transit, uint64_t* d_unrouted, hipStream_t st) {
    return ld_zero(c, flags, reinterpret_cast<uint64_t*>(d_edge), reinterpret_cast<uint64_t*>(d_transit), d_unrouted,
                   st);
}

// device accumulators of the blocking calls, as LoadsOut: the loads in double, unrouted in u64
struct EcmpOut {
    DevBuf de, dt, du;
    int m = 0, n = 0;
    int init(const shd_route* c) {
        m = c->m; n = c->n;
        int rc;
        if ((rc = de.alloc(sizeof(double) * (size_t)m)) || (rc = dt.alloc(sizeof(double) * (size_t)n)) ||
            (rc = du.alloc(sizeof(uint64_t))))
            return rc;
        if ((m && hipMemset(de.p, 0, sizeof(double) * (size_t)m) != hipSuccess) ||
            hipMemset(dt.p, 0, sizeof(double) * (size_t)n) != hipSuccess ||
            hipMemset(du.p, 0, sizeof(uint64_t)) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        return SHD_ROUTE_OK;
    }
    template <typename U>
    static int take(U* out, const void* dev, size_t count, bool add) {
        if (!add) return to_host(out, dev, sizeof(U) * count);
        if (!out || !count) return SHD_ROUTE_OK;
        std::vector<U> h(count);
        if (int rc = to_host(h.data(), dev, sizeof(U) * count)) return rc;
        for (size_t q = 0; q < count; q++) out[q] += h[q];
        return SHD_ROUTE_OK;
    }
    int finish(uint32_t flags, double* edge_out, double* transit_out, uint64_t* unrouted_out) {
        const bool add = (flags & SHD_ROUTE_LOADS_ADD) != 0;
        int rc;
        if ((rc = take(edge_out, de.p, (size_t)m, add)) || (rc = take(transit_out, dt.p, (size_t)n, add))) return rc;
        return take(unrouted_out, du.p, 1, add);
    }
    // ns sources on the null stream into the accumulators
    int add_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, const long long* d_eoff,
                    const void* d_wt, uint32_t flags) {
        return ec_sources(c, d_src, ns, d_tgt, nt, nt, d_eoff, (const uint64_t*)d_wt, flags, (double*)de.p,
                          (double*)dt.p, (uint64_t*)du.p, nullptr);
    }
};

// the outputs of a blocking call that has nothing to route
void ec_host_zero(const shd_route* c, uint32_t flags, double* edge_out, double* transit_out, uint64_t* unrouted_out) {
    if (flags & SHD_ROUTE_LOADS_ADD) return;
    if (edge_out) std::fill(edge_out, edge_out + c->m, 0.0);
    if (transit_out) std::fill(transit_out, transit_out + c->n, 0.0);
    if (unrouted_out) *unrouted_out = 0;
}

}  // namespace

extern "C" {

int shd_route_ecmp_loads_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                               int64_t ld, uint32_t flags, const uint64_t* d_wt, double* d_edge_load, double* d_transit,
                               uint64_t* d_unrouted, void* stream) {
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld)) return SHD_ROUTE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    int rc = ec_zero(c, flags, d_edge_load, d_transit, d_unrouted, st);
    if (rc || ns == 0 || nt == 0) return rc;
    return ec_sources(c, d_src, ns, d_tgt, nt, (long long)ld, nullptr, d_wt, flags, d_edge_load, d_transit, d_unrouted,
                      st);
}

int shd_route_ecmp_loads(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                         uint32_t flags, const uint64_t* wt, double* edge_load_out, double* transit_out,
                         uint64_t* unrouted_out) {
    if (!block_args_ok(c, src, ns, tgt, nt, nt)) return SHD_ROUTE_EINVAL;
    for (int32_t i = 0; i < ns; i++)
        if (src[i] < 0 || src[i] >= c->n) return SHD_ROUTE_EINVAL;
    for (int32_t j = 0; j < nt; j++)
        if (tgt[j] < 0 || tgt[j] >= c->n) return SHD_ROUTE_EINVAL;
    if (ns == 0 || nt == 0) {
        ec_host_zero(c, flags, edge_load_out, transit_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const size_t row_bytes = sizeof(uint64_t) * (size_t)nt;
    const int32_t chunk = host_chunk(ns, row_bytes);
    DevBuf dw;
    EcmpOut out;
    int rc;
    if ((wt && (rc = dw.alloc(row_bytes * chunk))) || (rc = out.init(c))) return rc;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t i0, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            if (wt && hipMemcpy(dw.p, wt + (size_t)i0 * nt, row_bytes * k, hipMemcpyHostToDevice) != hipSuccess)
                return SHD_ROUTE_EDEVICE;
            return out.add_sources(c, d_src, k, d_tgt, nt, nullptr, wt ? dw.p : nullptr, flags);
        },
        [&](int32_t i0, int32_t k) {
            return i0 + k < ns ? SHD_ROUTE_OK : out.finish(flags, edge_load_out, transit_out, unrouted_out);
        });
}

int shd_route_pair_ecmp_loads(shd_route_t* c, const int32_t* pair_src, const int32_t* pair_tgt,
                              const uint64_t* pair_wt, int64_t npairs, uint32_t flags, double* edge_load_out,
                              double* transit_out, uint64_t* unrouted_out) {
    if (!pair_args_ok(c, pair_src, pair_tgt, npairs) || !pairs_in_range(c, pair_src, pair_tgt, (int)npairs))
        return SHD_ROUTE_EINVAL;
    const int np = (int)npairs;
    if (np == 0) {
        ec_host_zero(c, flags, edge_load_out, transit_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    // the entries of distinct source u are the grouped positions first[u] .. first[u + 1]
    const PairGroups pg = group_pairs(pair_src, pair_tgt, pair_wt, np);
    const int nu = (int)pg.us.size();
    DevBuf dsrc, dtgt, dw, doff;
    EcmpOut out;
    int rc;
    if ((rc = dsrc.alloc(sizeof(int32_t) * nu)) || (rc = dtgt.alloc(sizeof(int32_t) * (size_t)np)) ||
        (pair_wt && (rc = dw.alloc(sizeof(uint64_t) * (size_t)np))) ||
        (rc = doff.alloc(sizeof(long long) * ((size_t)nu + 1))) || (rc = out.init(c)))
        return rc;
    if (hipMemcpy(dsrc.p, pg.us.data(), sizeof(int32_t) * nu, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dtgt.p, pg.gt.data(), sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess ||
        (pair_wt && hipMemcpy(dw.p, pg.gw.data(), sizeof(uint64_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(doff.p, pg.first.data(), sizeof(long long) * ((size_t)nu + 1), hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    SoftCode sc;
    if ((rc = out.add_sources(c, (const int32_t*)dsrc.p, nu, (const int32_t*)dtgt.p, 0, (const long long*)doff.p,
                              pair_wt ? dw.p : nullptr, flags)) ||
        (rc = sc.sync(c)) || (rc = out.finish(flags, edge_load_out, transit_out, unrouted_out)))
        return rc;
    return sc.soft;
}

}  // extern "C"

// ---- link loss ----
namespace {

// the per-element columns, once per context: 1.0f - loss and the loss as given of every edge
// id, the loss as given of every vertex (NaN = absent); the vertex factors are the context's
int ensure_loss(shd_route* c) {
    PathDev& p = c->path;
    if (p.lo_ready) return SHD_ROUTE_OK;
    int rc = ensure_hops(c);
    if (!rc) rc = upload(c, &p.lo_r, c->e_rel);
    if (!rc) rc = upload(c, &p.lo_q, c->e_loss);
    if (!rc) rc = upload(c, &p.lo_p, c->v_loss);
    if (!rc && loss_fits_lds(c->n))
        rc = hip_check(hipFuncSetAttribute((const void*)loss_tree_kernel<uint16_t, true, 1024>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLossLdsBudget));
    if (rc) return rc;
    p.lo_ready = 1;
    return SHD_ROUTE_OK;
}

// the sweeps of k sources and their entries (loss_tree_kernel); HBM slices as the loads', regrown as theirs
int lo_tree(shd_route* c, const uint32_t* par, const int32_t* hrow, const int32_t* d_src, int k, const int32_t* d_tgt,
            int nt, long long ld, const long long* d_eoff, const uint64_t* d_wt, int mode, const LossOuts& o,
            hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    const DevLoss q{c->path.lo_r, c->path.lo_q, c->d_vf, c->path.lo_p};
    const char* e = getenv("SHD_ROUTE_LOSS_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, mode, k, kLoSmall, LossLayout<uint16_t>::make(n).total, kLossLdsBudget,
                                     knob_off(e), a16(LossLayout<uint16_t>::make(n).total),
                                     a16(LossLayout<uint32_t>::make(n).total), hp_budget() / 4);
    return launch_state(c->path.lo_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((loss_tree_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g, q,
                           par, hrow, d_src, k, d_tgt, nt, ld, d_eoff, (const unsigned long long*)d_wt, mode, o, ws,
                           stride, c->d_err);
    });
}

// The loss of ns sources added into the outputs; entries as ld_sources takes them.
int lo_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, long long ld,
               const long long* d_eoff, const uint64_t* d_wt, uint32_t flags, const LossOuts& o, hipStream_t st) {
    int rc = ensure_loss(c);
    if (rc) return rc;
    const int mode = hp_mode(c, flags);
    return source_chunks(c, ns, mode, true, [&](int i0, int k, double* dist, uint32_t* par, int32_t* hrow) {
        if (par && (rc = hp_trees(c, d_src + i0, k, dist, par, hrow, st))) return rc;
        return lo_tree(c, par, hrow, d_src + i0, k, d_tgt, nt, ld, d_eoff ? d_eoff + i0 : nullptr,
                       d_wt && !d_eoff ? d_wt + (long long)i0 * ld : d_wt, mode, o, st);
    });
}

// zero the outputs a call without SHD_ROUTE_LOADS_ADD starts from (0.0 is all bits zero)
int lo_zero(shd_route* c, uint32_t flags, const LossOuts& o, hipStream_t st) {
    if (flags & SHD_ROUTE_LOADS_ADD) return SHD_ROUTE_OK;
    const size_t m8 = sizeof(double) * (size_t)c->m, n8 = sizeof(double) * (size_t)c->n;
    if ((o.edge_reach && m8 && hipMemsetAsync(o.edge_reach, 0, m8, st) != hipSuccess) ||
        (o.edge_drop && m8 && hipMemsetAsync(o.edge_drop, 0, m8, st) != hipSuccess) ||
        (o.vertex_drop && hipMemsetAsync(o.vertex_drop, 0, n8, st) != hipSuccess) ||
        (o.delivered && hipMemsetAsync(o.delivered, 0, n8, st) != hipSuccess) ||
        (o.unrouted && hipMemsetAsync(o.unrouted, 0, sizeof(uint64_t), st) != hipSuccess))
        return SHD_ROUTE_EDEVICE;
    return SHD_ROUTE_OK;
}

// the caller's host outputs of a blocking call
struct LossHost {
    double* edge_reach; double* edge_drop; double* vertex_drop; double* delivered;
    uint64_t* unrouted;
};

// device accumulators of the blocking calls, as LoadsOut: four columns in double, unrouted in u64
struct LossOut {
    DevBuf de, dd, dv, dl, du;
    int m = 0, n = 0;
    int init(const shd_route* c) {
        m = c->m; n = c->n;
        const size_t m8 = sizeof(double) * (size_t)m, n8 = sizeof(double) * (size_t)n;
        int rc;
        if ((rc = de.alloc(m8)) || (rc = dd.alloc(m8)) || (rc = dv.alloc(n8)) || (rc = dl.alloc(n8)) ||
            (rc = du.alloc(sizeof(uint64_t))))
            return rc;
        if ((m && (hipMemset(de.p, 0, m8) != hipSuccess || hipMemset(dd.p, 0, m8) != hipSuccess)) ||
            hipMemset(dv.p, 0, n8) != hipSuccess || hipMemset(dl.p, 0, n8) != hipSuccess ||
            hipMemset(du.p, 0, sizeof(uint64_t)) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        return SHD_ROUTE_OK;
    }
    LossOuts outs() const {
        return LossOuts{(double*)de.p, (double*)dd.p, (double*)dv.p, (double*)dl.p, (unsigned long long*)du.p};
    }
    int finish(uint32_t flags, const LossHost& h) {
        const bool add = (flags & SHD_ROUTE_LOADS_ADD) != 0;
        int rc;
        if ((rc = EcmpOut::take(h.edge_reach, de.p, (size_t)m, add)) ||
            (rc = EcmpOut::take(h.edge_drop, dd.p, (size_t)m, add)) ||
            (rc = EcmpOut::take(h.vertex_drop, dv.p, (size_t)n, add)) ||
            (rc = EcmpOut::take(h.delivered, dl.p, (size_t)n, add)))
            return rc;
        return EcmpOut::take(h.unrouted, du.p, 1, add);
    }
    // ns sources on the null stream into the accumulators
    int add_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, const long long* d_eoff,
                    const void* d_wt, uint32_t flags) {
        return lo_sources(c, d_src, ns, d_tgt, nt, nt, d_eoff, (const uint64_t*)d_wt, flags, outs(), nullptr);
    }
};

// the outputs of a blocking call that has nothing to route
void lo_host_zero(const shd_route* c, uint32_t flags, const LossHost& h) {
    if (flags & SHD_ROUTE_LOADS_ADD) return;
    if (h.edge_reach) std::fill(h.edge_reach, h.edge_reach + c->m, 0.0);
    if (h.edge_drop) std::fill(h.edge_drop, h.edge_drop + c->m, 0.0);
    if (h.vertex_drop) std::fill(h.vertex_drop, h.vertex_drop + c->n, 0.0);
    if (h.delivered) std::fill(h.delivered, h.delivered + c->n, 0.0);
    if (h.unrouted) *h.unrouted = 0;
}

}  // namespace

extern "C" {

int shd_route_loss_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                         int64_t ld, uint32_t flags, const uint64_t* d_wt, double* d_edge_reach, double* d_edge_drop,
                         double* d_vertex_drop, double* d_delivered, uint64_t* d_unrouted, void* stream) {
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld)) return SHD_ROUTE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const LossOuts o{d_edge_reach, d_edge_drop, d_vertex_drop, d_delivered, (unsigned long long*)d_unrouted};
    int rc = lo_zero(c, flags, o, st);
    if (rc || ns == 0 || nt == 0) return rc;
    return lo_sources(c, d_src, ns, d_tgt, nt, (long long)ld, nullptr, d_wt, flags, o, st);
}

int shd_route_loss(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, uint32_t flags,
                   const uint64_t* wt, double* edge_reach_out, double* edge_drop_out, double* vertex_drop_out,
                   double* delivered_out, uint64_t* unrouted_out) {
    if (!block_args_ok(c, src, ns, tgt, nt, nt)) return SHD_ROUTE_EINVAL;
    for (int32_t i = 0; i < ns; i++)
        if (src[i] < 0 || src[i] >= c->n) return SHD_ROUTE_EINVAL;
    for (int32_t j = 0; j < nt; j++)
        if (tgt[j] < 0 || tgt[j] >= c->n) return SHD_ROUTE_EINVAL;
    const LossHost h{edge_reach_out, edge_drop_out, vertex_drop_out, delivered_out, unrouted_out};
    if (ns == 0 || nt == 0) {
        lo_host_zero(c, flags, h);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const size_t row_bytes = sizeof(uint64_t) * (size_t)nt;
    const int32_t chunk = host_chunk(ns, row_bytes);
    DevBuf dw;
    LossOut out;
    int rc;
    if ((wt && (rc = dw.alloc(row_bytes * chunk))) || (rc = out.init(c))) return rc;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t i0, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            if (wt && hipMemcpy(dw.p, wt + (size_t)i0 * nt, row_bytes * k, hipMemcpyHostToDevice) != hipSuccess)
                return SHD_ROUTE_EDEVICE;
            return out.add_sources(c, d_src, k, d_tgt, nt, nullptr, wt ? dw.p : nullptr, flags);
        },
        [&](int32_t i0, int32_t k) { return i0 + k < ns ? SHD_ROUTE_OK : out.finish(flags, h); });
}

int shd_route_pair_loss(shd_route_t* c, const int32_t* pair_src, const int32_t* pair_tgt, const uint64_t* pair_wt,
                        int64_t npairs, uint32_t flags, double* edge_reach_out, double* edge_drop_out,
                        double* vertex_drop_out, double* delivered_out, uint64_t* unrouted_out) {
    if (!pair_args_ok(c, pair_src, pair_tgt, npairs) || !pairs_in_range(c, pair_src, pair_tgt, (int)npairs))
        return SHD_ROUTE_EINVAL;
    const int np = (int)npairs;
    const LossHost h{edge_reach_out, edge_drop_out, vertex_drop_out, delivered_out, unrouted_out};
    if (np == 0) {
        lo_host_zero(c, flags, h);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    // the entries of distinct source u are the grouped positions first[u] .. first[u + 1]
    const PairGroups pg = group_pairs(pair_src, pair_tgt, pair_wt, np);
    const int nu = (int)pg.us.size();
    DevBuf dsrc, dtgt, dw, doff;
    LossOut out;
    int rc;
    if ((rc = dsrc.alloc(sizeof(int32_t) * nu)) || (rc = dtgt.alloc(sizeof(int32_t) * (size_t)np)) ||
        (pair_wt && (rc = dw.alloc(sizeof(uint64_t) * (size_t)np))) ||
        (rc = doff.alloc(sizeof(long long) * ((size_t)nu + 1))) || (rc = out.init(c)))
        return rc;
    if (hipMemcpy(dsrc.p, pg.us.data(), sizeof(int32_t) * nu, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dtgt.p, pg.gt.data(), sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess ||
        (pair_wt && hipMemcpy(dw.p, pg.gw.data(), sizeof(uint64_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(doff.p, pg.first.data(), sizeof(long long) * ((size_t)nu + 1), hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    SoftCode sc;
    if ((rc = out.add_sources(c, (const int32_t*)dsrc.p, nu, (const int32_t*)dtgt.p, 0, (const long long*)doff.p,
                              pair_wt ? dw.p : nullptr, flags)) ||
        (rc = sc.sync(c)) || (rc = out.finish(flags, h)))
        return rc;
    return sc.soft;
}

}  // extern "C"

// ---- link outages ----
namespace {

// the per-element columns, once per context: the ends and the latency of every edge id and
// each vertex's self-loop edge ids, ascending
int ensure_outage(shd_route* c) {
    PathDev& p = c->path;
    if (p.ou_ready) return SHD_ROUTE_OK;
    const int n = c->n;
    std::vector<int> srow(n + 1, 0), seid;
    for (int e = 0; e < c->m; e++)
        if (c->e_src[e] == c->e_dst[e]) srow[c->e_src[e] + 1]++;
    for (int v = 0; v < n; v++) srow[v + 1] += srow[v];
    seid.resize(srow[n]);
    std::vector<int> fill(srow.begin(), srow.end() - 1);
    for (int e = 0; e < c->m; e++)
        if (c->e_src[e] == c->e_dst[e]) seid[fill[c->e_src[e]]++] = e;
    int rc = ensure_hops(c);
    if (!rc) rc = upload(c, &p.ou_ea, c->e_src);
    if (!rc) rc = upload(c, &p.ou_eb, c->e_dst);
    if (!rc) rc = upload(c, &p.ou_lat, c->e_lat);
    if (!rc) rc = upload(c, &p.ou_srow, srow);
    if (!rc) rc = upload(c, &p.ou_seid, seid);
    if (!rc && outage_fits_lds(n))
        rc = hip_check(hipFuncSetAttribute((const void*)outage_repair_kernel<uint16_t, true, 1024>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOutageLdsBudget));
    if (rc) return rc;
    p.ou_ready = 1;
    return SHD_ROUTE_OK;
}

struct OutageScn {  // the scenarios of a call on the device
    const int64_t* off;
    const int32_t* edge;
    int nscn;
};

DevOutage dev_outage(const shd_route* c, const OutageScn& s) {
    const PathDev& p = c->path;
    DevOutage q;
    q.m = c->m; q.directed = c->directed;
    q.ea = p.ou_ea; q.eb = p.ou_eb; q.lat = p.ou_lat; q.srow = p.ou_srow; q.seid = p.ou_seid;
    q.off = (const long long*)s.off; q.edge = s.edge; q.nscn = s.nscn;
    return q;
}

// the repairs of k sources and their entries over every scenario (outage_repair_kernel); the
// grid covers the units, HBM slices as the loads', regrown as theirs
int ou_repair(shd_route* c, const double* dist, const uint32_t* par, const int32_t* hrow, const int32_t* d_src, int k,
              const int32_t* d_tgt, int nt, long long ld, const long long* d_eoff, const uint64_t* d_wt,
              const OutageScn& scn, const OutageOuts& o, hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    const DevOutage q = dev_outage(c, scn);
    const OutageUnits U = OutageUnits::make(k, scn.nscn);
    const char* e = getenv("SHD_ROUTE_OUTAGE_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, 0, (int)std::min<long long>(U.units, 0x7FFFFFFF), kOuSmall,
                                     OutageLayout<uint16_t>::make(n).total, kOutageLdsBudget, knob_off(e),
                                     a16(OutageLayout<uint16_t>::make(n).total),
                                     a16(OutageLayout<uint32_t>::make(n).total), hp_budget() / 4);
    return launch_state(c->path.ou_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((outage_repair_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g, q,
                           U, dist, par, hrow, d_src, k, d_tgt, nt, ld, d_eoff, (const unsigned long long*)d_wt, o, ws,
                           stride, c->d_err);
    });
}

// The outages of ns sources added into the outputs; entries as ld_sources takes them.  The
// block's chunk i0 writes from row i0 of every plane of o.lat on.
int ou_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, long long ld,
               const long long* d_eoff, const uint64_t* d_wt, const OutageScn& scn, const OutageOuts& o,
               hipStream_t st) {
    int rc = ensure_outage(c);
    if (rc) return rc;
    return source_chunks(c, ns, 0, true, [&](int i0, int k, double* dist, uint32_t* par, int32_t* hrow) {
        if ((rc = hp_trees(c, d_src + i0, k, dist, par, hrow, st))) return rc;
        OutageOuts oc = o;
        if (oc.lat && !d_eoff) oc.lat += (long long)i0 * ld;
        return ou_repair(c, dist, par, hrow, d_src + i0, k, d_tgt, nt, ld, d_eoff ? d_eoff + i0 : nullptr,
                         d_wt && !d_eoff ? d_wt + (long long)i0 * ld : d_wt, scn, oc, st);
    });
}

// zero the statistics a call starts from (0.0 is all bits zero)
int ou_zero(const OutageOuts& o, int nscn, hipStream_t st) {
    const size_t sb = sizeof(uint64_t) * SHD_ROUTE_OUTAGE_NSTAT * (size_t)nscn;
    if ((o.stats && sb && hipMemsetAsync(o.stats, 0, sb, st) != hipSuccess) ||
        (o.max_add && nscn && hipMemsetAsync(o.max_add, 0, sizeof(double) * (size_t)nscn, st) != hipSuccess) ||
        (o.unrouted && hipMemsetAsync(o.unrouted, 0, sizeof(uint64_t), st) != hipSuccess))
        return SHD_ROUTE_EDEVICE;
    return SHD_ROUTE_OK;
}

// The scenarios of a blocking call: each list sorted ascending, on the device.
struct OutageHostScn {
    std::vector<int64_t> off;
    std::vector<int32_t> edge;
    DevBuf doff, dedge;
    // false: an offset that does not rise or an id that is no edge id
    bool take(const shd_route* c, const int64_t* scn_off, const int32_t* scn_edge, int32_t nscn) {
        if (nscn < 0 || (nscn && !scn_off)) return false;
        off.assign(1, 0);
        if (!nscn) return true;
        if (scn_off[0] != 0) return false;
        for (int k = 0; k < nscn; k++)
            if (scn_off[k + 1] < scn_off[k]) return false;
        const int64_t tot = scn_off[nscn];
        if (tot && !scn_edge) return false;
        for (int64_t x = 0; x < tot; x++)
            if (scn_edge[x] < 0 || scn_edge[x] >= c->m) return false;
        off.assign(scn_off, scn_off + nscn + 1);
        edge.assign(scn_edge, scn_edge + tot);
        for (int k = 0; k < nscn; k++) std::sort(edge.begin() + off[k], edge.begin() + off[k + 1]);
        return true;
    }
    int to_device() {
        int rc;
        if ((rc = doff.alloc(sizeof(int64_t) * off.size())) || (rc = dedge.alloc(sizeof(int32_t) * std::max<size_t>(edge.size(), 1))))
            return rc;
        if (hipMemcpy(doff.p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice) != hipSuccess ||
            (!edge.empty() &&
             hipMemcpy(dedge.p, edge.data(), sizeof(int32_t) * edge.size(), hipMemcpyHostToDevice) != hipSuccess))
            return SHD_ROUTE_EDEVICE;
        return SHD_ROUTE_OK;
    }
    OutageScn scn() const { return OutageScn{(const int64_t*)doff.p, (const int32_t*)dedge.p, (int)off.size() - 1}; }
};

// device accumulators of the blocking calls: the statistics, the maxima and unrouted
struct OutageOut {
    DevBuf ds, dm, du;
    int nscn = 0;
    int init(int nscn_) {
        nscn = nscn_;
        const size_t sb = sizeof(uint64_t) * SHD_ROUTE_OUTAGE_NSTAT * (size_t)std::max(nscn, 1);
        const size_t mb = sizeof(double) * (size_t)std::max(nscn, 1);
        int rc;
        if ((rc = ds.alloc(sb)) || (rc = dm.alloc(mb)) || (rc = du.alloc(sizeof(uint64_t)))) return rc;
        if (hipMemset(ds.p, 0, sb) != hipSuccess || hipMemset(dm.p, 0, mb) != hipSuccess ||
            hipMemset(du.p, 0, sizeof(uint64_t)) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        return SHD_ROUTE_OK;
    }
    OutageOuts outs(double* lat, long long plane) const {
        return OutageOuts{(unsigned long long*)ds.p, (unsigned long long*)dm.p, lat, plane, (unsigned long long*)du.p};
    }
    int finish(uint64_t* stats_out, double* max_add_out, uint64_t* unrouted_out) {
        int rc;
        if ((rc = to_host(stats_out, ds.p, sizeof(uint64_t) * SHD_ROUTE_OUTAGE_NSTAT * (size_t)nscn)) ||
            (rc = to_host(max_add_out, dm.p, sizeof(double) * (size_t)nscn)))
            return rc;
        return to_host(unrouted_out, du.p, sizeof(uint64_t));
    }
};

// the outputs of a blocking call that has nothing to route
void ou_host_zero(int32_t nscn, uint64_t* stats_out, double* max_add_out, uint64_t* unrouted_out) {
    if (stats_out) std::fill(stats_out, stats_out + (size_t)nscn * SHD_ROUTE_OUTAGE_NSTAT, (uint64_t)0);
    if (max_add_out) std::fill(max_add_out, max_add_out + nscn, 0.0);
    if (unrouted_out) *unrouted_out = 0;
}

}  // namespace

extern "C" {

int shd_route_outage_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                           int64_t ld, uint32_t flags, const uint64_t* d_wt, const int64_t* d_scn_off,
                           const int32_t* d_scn_edge, int32_t nscn, uint64_t* d_stats, double* d_max_add, double* d_lat,
                           uint64_t* d_unrouted, void* stream) {
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld) || flags != 0u || nscn < 0 || (nscn && !d_scn_off))
        return SHD_ROUTE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const OutageOuts o{(unsigned long long*)d_stats, (unsigned long long*)d_max_add, d_lat, (long long)ns * ld,
                       (unsigned long long*)d_unrouted};
    int rc = ou_zero(o, nscn, st);
    if (rc || ns == 0 || nt == 0) return rc;
    if ((rc = ensure_outage(c))) return rc;
    const OutageScn scn{d_scn_off, d_scn_edge, nscn};
    if (nscn) {
        hipLaunchKernelGGL(outage_check_kernel, dim3((unsigned)std::min((nscn + 255) / 256, 1024)), dim3(256), 0, st,
                           dev_outage(c, scn), c->d_err);
        if ((rc = hip_check(hipGetLastError()))) return rc;
    }
    return ou_sources(c, d_src, ns, d_tgt, nt, (long long)ld, nullptr, d_wt, scn, o, st);
}

int shd_route_outage(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, uint32_t flags,
                     const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge, int32_t nscn,
                     uint64_t* stats_out, double* max_add_out, double* lat_out, uint64_t* unrouted_out) {
    if (!block_args_ok(c, src, ns, tgt, nt, nt) || flags != 0u) return SHD_ROUTE_EINVAL;
    for (int32_t i = 0; i < ns; i++)
        if (src[i] < 0 || src[i] >= c->n) return SHD_ROUTE_EINVAL;
    for (int32_t j = 0; j < nt; j++)
        if (tgt[j] < 0 || tgt[j] >= c->n) return SHD_ROUTE_EINVAL;
    OutageHostScn hs;
    if (!hs.take(c, scn_off, scn_edge, nscn)) return SHD_ROUTE_EINVAL;
    if (ns == 0 || nt == 0) {
        ou_host_zero(nscn, stats_out, max_add_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const bool want_lat = lat_out && nscn;
    const size_t row_bytes = sizeof(uint64_t) * (size_t)nt;
    const int32_t chunk = host_chunk(ns, row_bytes * (want_lat ? (size_t)nscn + 1 : 1));
    DevBuf dw, dlat;
    OutageOut out;
    int rc;
    if ((wt && (rc = dw.alloc(row_bytes * chunk))) || (want_lat && (rc = dlat.alloc(row_bytes * chunk * nscn))) ||
        (rc = hs.to_device()) || (rc = out.init(nscn)))
        return rc;
    std::vector<double> stage;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t i0, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            if (wt && hipMemcpy(dw.p, wt + (size_t)i0 * nt, row_bytes * k, hipMemcpyHostToDevice) != hipSuccess)
                return SHD_ROUTE_EDEVICE;
            return ou_sources(c, d_src, k, d_tgt, nt, nt, nullptr, wt ? (const uint64_t*)dw.p : nullptr, hs.scn(),
                              out.outs(want_lat ? (double*)dlat.p : nullptr, (long long)k * nt), nullptr);
        },
        [&](int32_t i0, int32_t k) {
            if (want_lat) {  // the chunk's planes [scenario][k][nt] into the caller's [scenario][ns][nt]
                stage.resize((size_t)nscn * k * nt);
                if (int r = to_host(stage.data(), dlat.p, sizeof(double) * stage.size())) return r;
                for (int32_t q = 0; q < nscn; q++)
                    std::memcpy(lat_out + ((size_t)q * ns + i0) * nt, stage.data() + (size_t)q * k * nt, row_bytes * k);
            }
            return i0 + k < ns ? SHD_ROUTE_OK : out.finish(stats_out, max_add_out, unrouted_out);
        });
}

int shd_route_pair_outage(shd_route_t* c, const int32_t* pair_src, const int32_t* pair_tgt, const uint64_t* pair_wt,
                          int64_t npairs, uint32_t flags, const int64_t* scn_off, const int32_t* scn_edge, int32_t nscn,
                          uint64_t* stats_out, double* max_add_out, double* lat_out, uint64_t* unrouted_out) {
    if (!pair_args_ok(c, pair_src, pair_tgt, npairs) || !pairs_in_range(c, pair_src, pair_tgt, (int)npairs) ||
        flags != 0u)
        return SHD_ROUTE_EINVAL;
    OutageHostScn hs;
    if (!hs.take(c, scn_off, scn_edge, nscn)) return SHD_ROUTE_EINVAL;
    const int np = (int)npairs;
    if (np == 0) {
        ou_host_zero(nscn, stats_out, max_add_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    // the entries of distinct source u are the grouped positions first[u] .. first[u + 1]
    const PairGroups pg = group_pairs(pair_src, pair_tgt, pair_wt, np);
    const int nu = (int)pg.us.size();
    const bool want_lat = lat_out && nscn;
    DevBuf dsrc, dtgt, dw, doff, dlat;
    OutageOut out;
    int rc;
    if ((rc = dsrc.alloc(sizeof(int32_t) * nu)) || (rc = dtgt.alloc(sizeof(int32_t) * (size_t)np)) ||
        (pair_wt && (rc = dw.alloc(sizeof(uint64_t) * (size_t)np))) ||
        (rc = doff.alloc(sizeof(long long) * ((size_t)nu + 1))) ||
        (want_lat && (rc = dlat.alloc(sizeof(double) * (size_t)np * nscn))) || (rc = hs.to_device()) ||
        (rc = out.init(nscn)))
        return rc;
    if (hipMemcpy(dsrc.p, pg.us.data(), sizeof(int32_t) * nu, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dtgt.p, pg.gt.data(), sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess ||
        (pair_wt && hipMemcpy(dw.p, pg.gw.data(), sizeof(uint64_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(doff.p, pg.first.data(), sizeof(long long) * ((size_t)nu + 1), hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    SoftCode sc;
    if ((rc = ou_sources(c, (const int32_t*)dsrc.p, nu, (const int32_t*)dtgt.p, 0, 0, (const long long*)doff.p,
                         pair_wt ? (const uint64_t*)dw.p : nullptr, hs.scn(),
                         out.outs(want_lat ? (double*)dlat.p : nullptr, (long long)np), nullptr)) ||
        (rc = sc.sync(c)))
        return rc;
    if (want_lat) {  // back to the caller's pair order
        std::vector<double> grouped((size_t)np * nscn);
        if ((rc = to_host(grouped.data(), dlat.p, sizeof(double) * grouped.size()))) return rc;
        for (int32_t q = 0; q < nscn; q++)
            for (int gq = 0; gq < np; gq++) lat_out[(size_t)q * np + pg.order[gq]] = grouped[(size_t)q * np + gq];
    }
    if ((rc = out.finish(stats_out, max_add_out, unrouted_out))) return rc;
    return sc.soft;
}

}  // extern "C"

// ---- link repricing ----
namespace {

// what the outage and the ECMP loads calls build (edge ends, latencies, self-loop lists; the
// out-CSR with edge ids), the graph's own lo and hi of the absorbed-latency rule and the two
// words the check kernels reduce into, once per context
int ensure_reprice(shd_route* c) {
    PathDev& p = c->path;
    if (p.rp_ready) return SHD_ROUTE_OK;
    int rc = ensure_outage(c);
    if (!rc) rc = ensure_ecmp(c);
    if (rc) return rc;
    double lo = INFINITY, hi = 0.0;
    for (int e = 0; e < c->m; e++)
        if (c->e_src[e] != c->e_dst[e]) {
            lo = std::min(lo, c->e_lat[e]);
            hi = std::max(hi, c->e_lat[e]);
        }
    const std::vector<unsigned long long> z(2, 0ull);
    if ((rc = upload(c, &p.rp_lohi, z))) return rc;
    if (reprice_fits_lds(c->n))
        rc = hip_check(hipFuncSetAttribute((const void*)reprice_kernel<uint16_t, true, 1024>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOutageLdsBudget));
    if (rc) return rc;
    p.rp_lo = lo;
    p.rp_hi = hi;
    p.rp_ready = 1;
    return SHD_ROUTE_OK;
}

struct RepriceScn {  // the scenarios of a call on the device
    const int64_t* off;
    const int32_t* edge;
    const double* lat;
    int nscn;
};

DevReprice dev_reprice(const shd_route* c, const RepriceScn& s) {
    const PathDev& p = c->path;
    DevReprice r;
    r.o = dev_outage(c, OutageScn{s.off, s.edge, s.nscn});
    r.nlat = s.lat;
    r.row_out = p.ti_row; r.head_out = p.ti_head; r.w_out = p.ti_w; r.eid_out = p.ec_eid;
    return r;
}

unsigned long long f64_bits(double d) {
    unsigned long long b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

// the scenarios of k sources and their entries (reprice_kernel); the grid covers the units, HBM
// slices as the outages', regrown as theirs
int rp_units(shd_route* c, const double* dist, const uint32_t* par, const int32_t* hrow, const int32_t* d_src, int k,
             const int32_t* d_tgt, int nt, long long ld, const long long* d_eoff, const uint64_t* d_wt,
             const RepriceScn& scn, const RepriceOuts& o, hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    const DevReprice r = dev_reprice(c, scn);
    const OutageUnits U = OutageUnits::make(k, scn.nscn);
    const char* e = getenv("SHD_ROUTE_REPRICE_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, 0, (int)std::min<long long>(U.units, 0x7FFFFFFF), kRpSmall,
                                     RepriceLayout<uint16_t>::make(n).total, kOutageLdsBudget, knob_off(e),
                                     a16(RepriceLayout<uint16_t>::make(n).total),
                                     a16(RepriceLayout<uint32_t>::make(n).total), hp_budget() / 4);
    return launch_state(c->path.rp_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((reprice_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g, r, U,
                           dist, par, hrow, d_src, k, d_tgt, nt, ld, d_eoff, (const unsigned long long*)d_wt, o, ws,
                           stride, c->d_err);
    });
}

// The scenarios of ns sources added into the outputs; entries as ld_sources takes them.  The
// block's chunk i0 writes from row i0 of every plane of o.lat on.
int rp_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, long long ld,
               const long long* d_eoff, const uint64_t* d_wt, const RepriceScn& scn, const RepriceOuts& o,
               hipStream_t st) {
    int rc = ensure_reprice(c);
    if (rc) return rc;
    return source_chunks(c, ns, 0, true, [&](int i0, int k, double* dist, uint32_t* par, int32_t* hrow) {
        if ((rc = hp_trees(c, d_src + i0, k, dist, par, hrow, st))) return rc;
        RepriceOuts oc = o;
        if (oc.lat && !d_eoff) oc.lat += (long long)i0 * ld;
        return rp_units(c, dist, par, hrow, d_src + i0, k, d_tgt, nt, ld, d_eoff ? d_eoff + i0 : nullptr,
                        d_wt && !d_eoff ? d_wt + (long long)i0 * ld : d_wt, scn, oc, st);
    });
}

// what a call starts from: zero statistics and maxima (0.0 is all bits zero), +inf minima, and
// with lohi the graph's own lo and hi for the check kernels
int rp_zero(shd_route* c, const RepriceOuts& o, int nscn, bool lohi, hipStream_t st) {
    const size_t sb = sizeof(uint64_t) * SHD_ROUTE_REPRICE_NSTAT * (size_t)nscn;
    if ((o.stats && sb && hipMemsetAsync(o.stats, 0, sb, st) != hipSuccess) ||
        (o.max_add && nscn && hipMemsetAsync(o.max_add, 0, sizeof(double) * (size_t)nscn, st) != hipSuccess) ||
        (o.max_gain && nscn && hipMemsetAsync(o.max_gain, 0, sizeof(double) * (size_t)nscn, st) != hipSuccess) ||
        (o.unrouted && hipMemsetAsync(o.unrouted, 0, sizeof(uint64_t), st) != hipSuccess))
        return SHD_ROUTE_EDEVICE;
    if (!lohi && !(o.min_new && nscn)) return SHD_ROUTE_OK;
    const PathDev& p = c->path;
    hipLaunchKernelGGL(reprice_init_kernel, dim3((unsigned)std::min(std::max((nscn + 255) / 256, 1), 1024)), dim3(256), 0,
                       st, lohi ? p.rp_lohi : nullptr, f64_bits(p.rp_lo), f64_bits(p.rp_hi), o.min_new, nscn);
    return hip_check(hipGetLastError());
}

// The scenarios of a blocking call: each list sorted by id with its latencies, on the device.
struct RepriceHostScn {
    std::vector<int64_t> off;
    std::vector<int32_t> edge;
    std::vector<double> lat;
    DevBuf doff, dedge, dlat;
    // SHD_ROUTE_EINVAL: an offset that does not rise, an id that is no edge id or comes twice in
    // a scenario, a latency that is not finite and > 0; SHD_ROUTE_EUNSUPPORTED: the
    // absorbed-latency rule over the graph's lo and hi and every new latency
    int take(const shd_route* c, double lo, double hi, const int64_t* scn_off, const int32_t* scn_edge,
             const double* scn_lat, int32_t nscn) {
        if (nscn < 0 || (nscn && !scn_off)) return SHD_ROUTE_EINVAL;
        off.assign(1, 0);
        if (!nscn) return SHD_ROUTE_OK;
        if (scn_off[0] != 0) return SHD_ROUTE_EINVAL;
        for (int k = 0; k < nscn; k++)
            if (scn_off[k + 1] < scn_off[k]) return SHD_ROUTE_EINVAL;
        const int64_t tot = scn_off[nscn];
        if (tot && (!scn_edge || !scn_lat)) return SHD_ROUTE_EINVAL;
        for (int64_t x = 0; x < tot; x++)
            if (scn_edge[x] < 0 || scn_edge[x] >= c->m || !(scn_lat[x] > 0.0) || std::isinf(scn_lat[x]))
                return SHD_ROUTE_EINVAL;
        off.assign(scn_off, scn_off + nscn + 1);
        edge.resize(tot);
        lat.resize(tot);
        std::vector<int64_t> idx;
        for (int k = 0; k < nscn; k++) {
            idx.resize(off[k + 1] - off[k]);
            std::iota(idx.begin(), idx.end(), off[k]);
            std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return scn_edge[a] < scn_edge[b]; });
            for (size_t y = 0; y < idx.size(); y++) {
                if (y && scn_edge[idx[y]] == scn_edge[idx[y - 1]]) return SHD_ROUTE_EINVAL;
                edge[off[k] + y] = scn_edge[idx[y]];
                lat[off[k] + y] = scn_lat[idx[y]];
            }
        }
        for (int64_t x = 0; x < tot; x++)
            if (c->e_src[edge[x]] != c->e_dst[edge[x]]) {
                lo = std::min(lo, lat[x]);
                hi = std::max(hi, lat[x]);
            }
        if (hi > 0.0 && lo <= (double)(c->n - 1) * (hi * 0x1p-52)) return SHD_ROUTE_EUNSUPPORTED;
        return SHD_ROUTE_OK;
    }
    int to_device() {
        int rc;
        const size_t ne = std::max<size_t>(edge.size(), 1);
        if ((rc = doff.alloc(sizeof(int64_t) * off.size())) || (rc = dedge.alloc(sizeof(int32_t) * ne)) ||
            (rc = dlat.alloc(sizeof(double) * ne)))
            return rc;
        if (hipMemcpy(doff.p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice) != hipSuccess ||
            (!edge.empty() &&
             (hipMemcpy(dedge.p, edge.data(), sizeof(int32_t) * edge.size(), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(dlat.p, lat.data(), sizeof(double) * lat.size(), hipMemcpyHostToDevice) != hipSuccess)))
            return SHD_ROUTE_EDEVICE;
        return SHD_ROUTE_OK;
    }
    RepriceScn scn() const {
        return RepriceScn{(const int64_t*)doff.p, (const int32_t*)dedge.p, (const double*)dlat.p, (int)off.size() - 1};
    }
};

// the graph's own lo and hi without a device: what take() starts from
void rp_graph_lohi(const shd_route* c, double* lo, double* hi) {
    *lo = INFINITY;
    *hi = 0.0;
    for (int e = 0; e < c->m; e++)
        if (c->e_src[e] != c->e_dst[e]) {
            *lo = std::min(*lo, c->e_lat[e]);
            *hi = std::max(*hi, c->e_lat[e]);
        }
}

// device accumulators of the blocking calls: the statistics, the maxima, the minima and unrouted
struct RepriceOut {
    DevBuf ds, dm, dg, dn, du;
    int nscn = 0;
    int init(shd_route* c, int nscn_) {
        nscn = nscn_;
        const size_t sb = sizeof(uint64_t) * SHD_ROUTE_REPRICE_NSTAT * (size_t)std::max(nscn, 1);
        const size_t mb = sizeof(double) * (size_t)std::max(nscn, 1);
        int rc;
        if ((rc = ds.alloc(sb)) || (rc = dm.alloc(mb)) || (rc = dg.alloc(mb)) || (rc = dn.alloc(mb)) ||
            (rc = du.alloc(sizeof(uint64_t))))
            return rc;
        return rp_zero(c, outs(nullptr, 0), nscn, false, nullptr);
    }
    RepriceOuts outs(double* lat, long long plane) const {
        return RepriceOuts{(unsigned long long*)ds.p, (unsigned long long*)dm.p, (unsigned long long*)dg.p,
                           (unsigned long long*)dn.p, lat, plane, (unsigned long long*)du.p};
    }
    int finish(uint64_t* stats_out, double* max_add_out, double* max_gain_out, double* min_new_out,
               uint64_t* unrouted_out) {
        int rc;
        if ((rc = to_host(stats_out, ds.p, sizeof(uint64_t) * SHD_ROUTE_REPRICE_NSTAT * (size_t)nscn)) ||
            (rc = to_host(max_add_out, dm.p, sizeof(double) * (size_t)nscn)) ||
            (rc = to_host(max_gain_out, dg.p, sizeof(double) * (size_t)nscn)) ||
            (rc = to_host(min_new_out, dn.p, sizeof(double) * (size_t)nscn)))
            return rc;
        return to_host(unrouted_out, du.p, sizeof(uint64_t));
    }
};

// the outputs of a blocking call that has nothing to route
void rp_host_zero(int32_t nscn, uint64_t* stats_out, double* max_add_out, double* max_gain_out, double* min_new_out,
                  uint64_t* unrouted_out) {
    if (stats_out) std::fill(stats_out, stats_out + (size_t)nscn * SHD_ROUTE_REPRICE_NSTAT, (uint64_t)0);
    if (max_add_out) std::fill(max_add_out, max_add_out + nscn, 0.0);
    if (max_gain_out) std::fill(max_gain_out, max_gain_out + nscn, 0.0);
    if (min_new_out) std::fill(min_new_out, min_new_out + nscn, (double)INFINITY);
    if (unrouted_out) *unrouted_out = 0;
}

}  // namespace

extern "C" {

int shd_route_reprice_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                            int64_t ld, uint32_t flags, const uint64_t* d_wt, const int64_t* d_scn_off,
                            const int32_t* d_scn_edge, const double* d_scn_lat, int32_t nscn, uint64_t* d_stats,
                            double* d_max_add, double* d_max_gain, double* d_min_new, double* d_lat,
                            uint64_t* d_unrouted, void* stream) {
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld) || flags != 0u || nscn < 0 || (nscn && !d_scn_off))
        return SHD_ROUTE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const RepriceOuts o{(unsigned long long*)d_stats, (unsigned long long*)d_max_add, (unsigned long long*)d_max_gain,
                        (unsigned long long*)d_min_new, d_lat, (long long)ns * ld, (unsigned long long*)d_unrouted};
    int rc = ensure_reprice(c);
    if (rc) return rc;
    if ((rc = rp_zero(c, o, nscn, nscn > 0, st)) || ns == 0 || nt == 0) return rc;
    const RepriceScn scn{d_scn_off, d_scn_edge, d_scn_lat, nscn};
    if (nscn) {
        hipLaunchKernelGGL(reprice_check_kernel, dim3((unsigned)std::min((nscn + 255) / 256, 1024)), dim3(256), 0, st,
                           dev_reprice(c, scn), c->path.rp_lohi, c->d_err);
        hipLaunchKernelGGL(reprice_absorb_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)c->path.rp_lohi,
                           c->n, c->d_err);
        if ((rc = hip_check(hipGetLastError()))) return rc;
    }
    return rp_sources(c, d_src, ns, d_tgt, nt, (long long)ld, nullptr, d_wt, scn, o, st);
}

int shd_route_reprice(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, uint32_t flags,
                      const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge, const double* scn_lat,
                      int32_t nscn, uint64_t* stats_out, double* max_add_out, double* max_gain_out,
                      double* min_new_out, double* lat_out, uint64_t* unrouted_out) {
    if (!block_args_ok(c, src, ns, tgt, nt, nt) || flags != 0u) return SHD_ROUTE_EINVAL;
    for (int32_t i = 0; i < ns; i++)
        if (src[i] < 0 || src[i] >= c->n) return SHD_ROUTE_EINVAL;
    for (int32_t j = 0; j < nt; j++)
        if (tgt[j] < 0 || tgt[j] >= c->n) return SHD_ROUTE_EINVAL;
    RepriceHostScn hs;
    double lo, hi;
    rp_graph_lohi(c, &lo, &hi);
    int rc;
    if ((rc = hs.take(c, lo, hi, scn_off, scn_edge, scn_lat, nscn))) return rc;
    if (ns == 0 || nt == 0) {
        rp_host_zero(nscn, stats_out, max_add_out, max_gain_out, min_new_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((rc = ensure_reprice(c))) return rc;
    const bool want_lat = lat_out && nscn;
    const size_t row_bytes = sizeof(uint64_t) * (size_t)nt;
    const int32_t chunk = host_chunk(ns, row_bytes * (want_lat ? (size_t)nscn + 1 : 1));
    DevBuf dw, dlat;
    RepriceOut out;
    if ((wt && (rc = dw.alloc(row_bytes * chunk))) || (want_lat && (rc = dlat.alloc(row_bytes * chunk * nscn))) ||
        (rc = hs.to_device()) || (rc = out.init(c, nscn)))
        return rc;
    std::vector<double> stage;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t i0, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            if (wt && hipMemcpy(dw.p, wt + (size_t)i0 * nt, row_bytes * k, hipMemcpyHostToDevice) != hipSuccess)
                return SHD_ROUTE_EDEVICE;
            return rp_sources(c, d_src, k, d_tgt, nt, nt, nullptr, wt ? (const uint64_t*)dw.p : nullptr, hs.scn(),
                              out.outs(want_lat ? (double*)dlat.p : nullptr, (long long)k * nt), nullptr);
        },
        [&](int32_t i0, int32_t k) {
            if (want_lat) {  // the chunk's planes [scenario][k][nt] into the caller's [scenario][ns][nt]
                stage.resize((size_t)nscn * k * nt);
                if (int r = to_host(stage.data(), dlat.p, sizeof(double) * stage.size())) return r;
                for (int32_t q = 0; q < nscn; q++)
                    std::memcpy(lat_out + ((size_t)q * ns + i0) * nt, stage.data() + (size_t)q * k * nt, row_bytes * k);
            }
            return i0 + k < ns ? SHD_ROUTE_OK
                               : out.finish(stats_out, max_add_out, max_gain_out, min_new_out, unrouted_out);
        });
}

int shd_route_pair_reprice(shd_route_t* c, const int32_t* pair_src, const int32_t* pair_tgt, const uint64_t* pair_wt,
                           int64_t npairs, uint32_t flags, const int64_t* scn_off, const int32_t* scn_edge,
                           const double* scn_lat, int32_t nscn, uint64_t* stats_out, double* max_add_out,
                           double* max_gain_out, double* min_new_out, double* lat_out, uint64_t* unrouted_out) {
    if (!pair_args_ok(c, pair_src, pair_tgt, npairs) || !pairs_in_range(c, pair_src, pair_tgt, (int)npairs) ||
        flags != 0u)
        return SHD_ROUTE_EINVAL;
    RepriceHostScn hs;
    double lo, hi;
    rp_graph_lohi(c, &lo, &hi);
    int rc;
    if ((rc = hs.take(c, lo, hi, scn_off, scn_edge, scn_lat, nscn))) return rc;
    const int np = (int)npairs;
    if (np == 0) {
        rp_host_zero(nscn, stats_out, max_add_out, max_gain_out, min_new_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((rc = ensure_reprice(c))) return rc;
    // the entries of distinct source u are the grouped positions first[u] .. first[u + 1]
    const PairGroups pg = group_pairs(pair_src, pair_tgt, pair_wt, np);
    const int nu = (int)pg.us.size();
    const bool want_lat = lat_out && nscn;
    DevBuf dsrc, dtgt, dw, doff, dlat;
    RepriceOut out;
    if ((rc = dsrc.alloc(sizeof(int32_t) * nu)) || (rc = dtgt.alloc(sizeof(int32_t) * (size_t)np)) ||
        (pair_wt && (rc = dw.alloc(sizeof(uint64_t) * (size_t)np))) ||
        (rc = doff.alloc(sizeof(long long) * ((size_t)nu + 1))) ||
        (want_lat && (rc = dlat.alloc(sizeof(double) * (size_t)np * nscn))) || (rc = hs.to_device()) ||
        (rc = out.init(c, nscn)))
        return rc;
    if (hipMemcpy(dsrc.p, pg.us.data(), sizeof(int32_t) * nu, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dtgt.p, pg.gt.data(), sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess ||
        (pair_wt && hipMemcpy(dw.p, pg.gw.data(), sizeof(uint64_t) * (size_t)np, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(doff.p, pg.first.data(), sizeof(long long) * ((size_t)nu + 1), hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    SoftCode sc;
    if ((rc = rp_sources(c, (const int32_t*)dsrc.p, nu, (const int32_t*)dtgt.p, 0, 0, (const long long*)doff.p,
                         pair_wt ? (const uint64_t*)dw.p : nullptr, hs.scn(),
                         out.outs(want_lat ? (double*)dlat.p : nullptr, (long long)np), nullptr)) ||
        (rc = sc.sync(c)))
        return rc;
    if (want_lat) {  // back to the caller's pair order
        std::vector<double> grouped((size_t)np * nscn);
        if ((rc = to_host(grouped.data(), dlat.p, sizeof(double) * grouped.size()))) return rc;
        for (int32_t q = 0; q < nscn; q++)
            for (int gq = 0; gq < np; gq++) lat_out[(size_t)q * np + pg.order[gq]] = grouped[(size_t)q * np + gq];
    }
    if ((rc = out.finish(stats_out, max_add_out, max_gain_out, min_new_out, unrouted_out))) return rc;
    return sc.soft;
}

}  // extern "C"
