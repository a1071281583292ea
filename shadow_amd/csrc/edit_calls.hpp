// edit_calls.hpp -- the link edit calls of include/shd_route.h (shd_route_edit_async,
// shd_route_edit, shd_route_pair_edit) over link_edit.hpp.  Included by engine.hip behind
// path_calls.hpp, whose host stages (source chunks, state forms, the outage and repricing
// columns, the host blocks and pair groups) it uses as they are; what the host forms decide
// without a device is edit_host.hpp.
#include "edit_host.hpp"

// ---- link edits ----
namespace {

// what the repricing calls build, the two words the check kernel reduces into and the raised
// dynamic-LDS limit, once per context
int ensure_edit(shd_route* c) {
    PathDev& p = c->path;
    if (p.ed_ready) return SHD_ROUTE_OK;
    int rc = ensure_reprice(c);
    if (rc) return rc;
    const std::vector<unsigned long long> z(2, 0ull);
    if ((rc = upload(c, &p.ed_lohi, z))) return rc;
    if (reprice_fits_lds(c->n))
        rc = hip_check(hipFuncSetAttribute((const void*)edit_kernel<uint16_t, true, 1024>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kOutageLdsBudget));
    if (rc) return rc;
    p.ed_ready = 1;
    return SHD_ROUTE_OK;
}

struct EditScn {  // the scenarios of a call on the device
    const int64_t* off;
    const int32_t* edge;
    const int32_t* a;
    const int32_t* b;
    const double* lat;
    int nscn;
};

DevEdit dev_edit(const shd_route* c, const EditScn& s) {
    DevEdit e;
    e.r = dev_reprice(c, RepriceScn{s.off, s.edge, s.lat, s.nscn});
    e.sa = s.a;
    e.sb = s.b;
    return e;
}

// the scenarios of k sources and their entries (edit_kernel); the grid covers the units, HBM
// slices as the repricing's, regrown as theirs
int ed_units(shd_route* c, const double* dist, const uint32_t* par, const int32_t* hrow, const int32_t* d_src, int k,
             const int32_t* d_tgt, int nt, long long ld, const long long* d_eoff, const uint64_t* d_wt,
             const EditScn& scn, const EditOuts& o, hipStream_t st) {
    const int n = c->n;
    const DevHops g = dev_hops(c);
    const DevEdit ed = dev_edit(c, scn);
    const OutageUnits U = OutageUnits::make(k, scn.nscn);
    const char* e = getenv("SHD_ROUTE_EDIT_LDS");  // "0": the HBM form on graphs the LDS form takes
    const StateLaunch f = state_form(n, 0, (int)std::min<long long>(U.units, 0x7FFFFFFF), kEdSmall,
                                     RepriceLayout<uint16_t>::make(n).total, kOutageLdsBudget, knob_off(e),
                                     a16(RepriceLayout<uint16_t>::make(n).total),
                                     a16(RepriceLayout<uint32_t>::make(n).total), hp_budget() / 4);
    return launch_state(c->path.ed_ws, f, st, [&](auto tag, char* ws, size_t stride) {
        using F = decltype(tag);
        hipLaunchKernelGGL((edit_kernel<typename F::t, F::lds, 1024>), dim3(f.grid), dim3(1024), f.lds, st, g, ed, U,
                           dist, par, hrow, d_src, k, d_tgt, nt, ld, d_eoff, (const unsigned long long*)d_wt, o, ws,
                           stride, c->d_err);
    });
}

// The scenarios of ns sources added into the outputs; entries as ld_sources takes them.  The
// block's chunk i0 writes from row i0 of every plane of o.lat on.
int ed_sources(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, long long ld,
               const long long* d_eoff, const uint64_t* d_wt, const EditScn& scn, const EditOuts& o, hipStream_t st) {
    int rc = ensure_edit(c);
    if (rc) return rc;
    return source_chunks(c, ns, 0, true, [&](int i0, int k, double* dist, uint32_t* par, int32_t* hrow) {
        if ((rc = hp_trees(c, d_src + i0, k, dist, par, hrow, st))) return rc;
        EditOuts oc = o;
        if (oc.lat && !d_eoff) oc.lat += (long long)i0 * ld;
        return ed_units(c, dist, par, hrow, d_src + i0, k, d_tgt, nt, ld, d_eoff ? d_eoff + i0 : nullptr,
                        d_wt && !d_eoff ? d_wt + (long long)i0 * ld : d_wt, scn, oc, st);
    });
}

// what a call starts from: zero statistics and maxima (0.0 is all bits zero), +inf minima, and
// with lohi the graph's own lo and hi for the check kernel
int ed_zero(shd_route* c, const EditOuts& o, int nscn, bool lohi, hipStream_t st) {
    const size_t sb = sizeof(uint64_t) * SHD_ROUTE_EDIT_NSTAT * (size_t)nscn;
    if ((o.stats && sb && hipMemsetAsync(o.stats, 0, sb, st) != hipSuccess) ||
        (o.max_add && nscn && hipMemsetAsync(o.max_add, 0, sizeof(double) * (size_t)nscn, st) != hipSuccess) ||
        (o.max_gain && nscn && hipMemsetAsync(o.max_gain, 0, sizeof(double) * (size_t)nscn, st) != hipSuccess) ||
        (o.unrouted && hipMemsetAsync(o.unrouted, 0, sizeof(uint64_t), st) != hipSuccess))
        return SHD_ROUTE_EDEVICE;
    if (!lohi && !(o.min_new && nscn)) return SHD_ROUTE_OK;
    const PathDev& p = c->path;
    hipLaunchKernelGGL(reprice_init_kernel, dim3((unsigned)std::min(std::max((nscn + 255) / 256, 1), 1024)), dim3(256), 0,
                       st, lohi ? p.ed_lohi : nullptr, f64_bits(p.rp_lo), f64_bits(p.rp_hi), o.min_new, nscn);
    return hip_check(hipGetLastError());
}

// The scenarios of a blocking call (edit_host.hpp) on the device.
struct EditDevScn {
    EditHostScn h;
    DevBuf doff, dedge, da, db, dlat;
    int take(const shd_route* c, const int64_t* scn_off, const int32_t* scn_edge, const int32_t* scn_a,
             const int32_t* scn_b, const double* scn_lat, int32_t nscn) {
        double lo, hi;
        edit_graph_lohi(c->m, c->e_src.data(), c->e_dst.data(), c->e_lat.data(), &lo, &hi);
        return h.take(c->n, c->m, c->e_src.data(), c->e_dst.data(), lo, hi, scn_off, scn_edge, scn_a, scn_b, scn_lat,
                      nscn);
    }
    int to_device() {
        int rc;
        const size_t ne = std::max<size_t>(h.edge.size(), 1);
        if ((rc = doff.alloc(sizeof(int64_t) * h.off.size())) || (rc = dedge.alloc(sizeof(int32_t) * ne)) ||
            (rc = da.alloc(sizeof(int32_t) * ne)) || (rc = db.alloc(sizeof(int32_t) * ne)) ||
            (rc = dlat.alloc(sizeof(double) * ne)))
            return rc;
        const size_t ib = sizeof(int32_t) * h.edge.size();
        if (hipMemcpy(doff.p, h.off.data(), sizeof(int64_t) * h.off.size(), hipMemcpyHostToDevice) != hipSuccess ||
            (!h.edge.empty() &&
             (hipMemcpy(dedge.p, h.edge.data(), ib, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(da.p, h.a.data(), ib, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(db.p, h.b.data(), ib, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(dlat.p, h.lat.data(), sizeof(double) * h.lat.size(), hipMemcpyHostToDevice) != hipSuccess)))
            return SHD_ROUTE_EDEVICE;
        return SHD_ROUTE_OK;
    }
    EditScn scn() const {
        return EditScn{(const int64_t*)doff.p, (const int32_t*)dedge.p, (const int32_t*)da.p, (const int32_t*)db.p,
                       (const double*)dlat.p, (int)h.off.size() - 1};
    }
};

// device accumulators of the blocking calls: the statistics, the maxima, the minima and unrouted
struct EditOut {
    DevBuf ds, dm, dg, dn, du;
    int nscn = 0;
    int init(shd_route* c, int nscn_) {
        nscn = nscn_;
        const size_t sb = sizeof(uint64_t) * SHD_ROUTE_EDIT_NSTAT * (size_t)std::max(nscn, 1);
        const size_t mb = sizeof(double) * (size_t)std::max(nscn, 1);
        int rc;
        if ((rc = ds.alloc(sb)) || (rc = dm.alloc(mb)) || (rc = dg.alloc(mb)) || (rc = dn.alloc(mb)) ||
            (rc = du.alloc(sizeof(uint64_t))))
            return rc;
        return ed_zero(c, outs(nullptr, 0), nscn, false, nullptr);
    }
    EditOuts outs(double* lat, long long plane) const {
        return EditOuts{(unsigned long long*)ds.p, (unsigned long long*)dm.p, (unsigned long long*)dg.p,
                        (unsigned long long*)dn.p, lat, plane, (unsigned long long*)du.p};
    }
    int finish(uint64_t* stats_out, double* max_add_out, double* max_gain_out, double* min_new_out,
               uint64_t* unrouted_out) {
        int rc;
        if ((rc = to_host(stats_out, ds.p, sizeof(uint64_t) * SHD_ROUTE_EDIT_NSTAT * (size_t)nscn)) ||
            (rc = to_host(max_add_out, dm.p, sizeof(double) * (size_t)nscn)) ||
            (rc = to_host(max_gain_out, dg.p, sizeof(double) * (size_t)nscn)) ||
            (rc = to_host(min_new_out, dn.p, sizeof(double) * (size_t)nscn)))
            return rc;
        return to_host(unrouted_out, du.p, sizeof(uint64_t));
    }
};

// the outputs of a blocking call that has nothing to route
void ed_host_zero(int32_t nscn, uint64_t* stats_out, double* max_add_out, double* max_gain_out, double* min_new_out,
                  uint64_t* unrouted_out) {
    if (stats_out) std::fill(stats_out, stats_out + (size_t)nscn * SHD_ROUTE_EDIT_NSTAT, (uint64_t)0);
    if (max_add_out) std::fill(max_add_out, max_add_out + nscn, 0.0);
    if (max_gain_out) std::fill(max_gain_out, max_gain_out + nscn, 0.0);
    if (min_new_out) std::fill(min_new_out, min_new_out + nscn, (double)INFINITY);
    if (unrouted_out) *unrouted_out = 0;
}

}  // namespace

extern "C" {

int shd_route_edit_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt, int64_t ld,
                         uint32_t flags, const uint64_t* d_wt, const int64_t* d_scn_off, const int32_t* d_scn_edge,
                         const int32_t* d_scn_a, const int32_t* d_scn_b, const double* d_scn_lat, int32_t nscn,
                         uint64_t* d_stats, double* d_max_add, double* d_max_gain, double* d_min_new, double* d_lat,
                         uint64_t* d_unrouted, void* stream) {
    if (!block_args_ok(c, d_src, ns, d_tgt, nt, ld) || flags != 0u || nscn < 0 || (nscn && !d_scn_off))
        return SHD_ROUTE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const EditOuts o{(unsigned long long*)d_stats, (unsigned long long*)d_max_add, (unsigned long long*)d_max_gain,
                     (unsigned long long*)d_min_new, d_lat, (long long)ns * ld, (unsigned long long*)d_unrouted};
    int rc = ensure_edit(c);
    if (rc) return rc;
    if ((rc = ed_zero(c, o, nscn, nscn > 0, st)) || ns == 0 || nt == 0) return rc;
    const EditScn scn{d_scn_off, d_scn_edge, d_scn_a, d_scn_b, d_scn_lat, nscn};
    if (nscn) {
        hipLaunchKernelGGL(edit_check_kernel, dim3((unsigned)std::min((nscn + 255) / 256, 1024)), dim3(256), 0, st,
                           dev_edit(c, scn), c->n, c->path.ed_lohi, c->d_err);
        hipLaunchKernelGGL(reprice_absorb_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)c->path.ed_lohi,
                           c->n, c->d_err);
        if ((rc = hip_check(hipGetLastError()))) return rc;
    }
    return ed_sources(c, d_src, ns, d_tgt, nt, (long long)ld, nullptr, d_wt, scn, o, st);
}

int shd_route_edit(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, uint32_t flags,
                   const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge, const int32_t* scn_a,
                   const int32_t* scn_b, const double* scn_lat, int32_t nscn, uint64_t* stats_out, double* max_add_out,
                   double* max_gain_out, double* min_new_out, double* lat_out, uint64_t* unrouted_out) {
    if (!block_args_ok(c, src, ns, tgt, nt, nt) || flags != 0u) return SHD_ROUTE_EINVAL;
    for (int32_t i = 0; i < ns; i++)
        if (src[i] < 0 || src[i] >= c->n) return SHD_ROUTE_EINVAL;
    for (int32_t j = 0; j < nt; j++)
        if (tgt[j] < 0 || tgt[j] >= c->n) return SHD_ROUTE_EINVAL;
    EditDevScn hs;
    int rc;
    if ((rc = hs.take(c, scn_off, scn_edge, scn_a, scn_b, scn_lat, nscn))) return rc;
    if (ns == 0 || nt == 0) {
        ed_host_zero(nscn, stats_out, max_add_out, max_gain_out, min_new_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((rc = ensure_edit(c))) return rc;
    const bool want_lat = lat_out && nscn;
    const size_t row_bytes = sizeof(uint64_t) * (size_t)nt;
    const int32_t chunk = host_chunk(ns, row_bytes * (want_lat ? (size_t)nscn + 1 : 1));
    DevBuf dw, dlat;
    EditOut out;
    if ((wt && (rc = dw.alloc(row_bytes * chunk))) || (want_lat && (rc = dlat.alloc(row_bytes * chunk * nscn))) ||
        (rc = hs.to_device()) || (rc = out.init(c, nscn)))
        return rc;
    std::vector<double> stage;
    return host_blocks(
        c, src, ns, tgt, nt, chunk,
        [&](int32_t i0, int32_t k, const int32_t* d_src, const int32_t* d_tgt) {
            if (wt && hipMemcpy(dw.p, wt + (size_t)i0 * nt, row_bytes * k, hipMemcpyHostToDevice) != hipSuccess)
                return SHD_ROUTE_EDEVICE;
            return ed_sources(c, d_src, k, d_tgt, nt, nt, nullptr, wt ? (const uint64_t*)dw.p : nullptr, hs.scn(),
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

int shd_route_pair_edit(shd_route_t* c, const int32_t* pair_src, const int32_t* pair_tgt, const uint64_t* pair_wt,
                        int64_t npairs, uint32_t flags, const int64_t* scn_off, const int32_t* scn_edge,
                        const int32_t* scn_a, const int32_t* scn_b, const double* scn_lat, int32_t nscn,
                        uint64_t* stats_out, double* max_add_out, double* max_gain_out, double* min_new_out,
                        double* lat_out, uint64_t* unrouted_out) {
    if (!pair_args_ok(c, pair_src, pair_tgt, npairs) || !pairs_in_range(c, pair_src, pair_tgt, (int)npairs) ||
        flags != 0u)
        return SHD_ROUTE_EINVAL;
    EditDevScn hs;
    int rc;
    if ((rc = hs.take(c, scn_off, scn_edge, scn_a, scn_b, scn_lat, nscn))) return rc;
    const int np = (int)npairs;
    if (np == 0) {
        ed_host_zero(nscn, stats_out, max_add_out, max_gain_out, min_new_out, unrouted_out);
        return SHD_ROUTE_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((rc = ensure_edit(c))) return rc;
    // the entries of distinct source u are the grouped positions first[u] .. first[u + 1]
    const PairGroups pg = group_pairs(pair_src, pair_tgt, pair_wt, np);
    const int nu = (int)pg.us.size();
    const bool want_lat = lat_out && nscn;
    DevBuf dsrc, dtgt, dw, doff, dlat;
    EditOut out;
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
    if ((rc = ed_sources(c, (const int32_t*)dsrc.p, nu, (const int32_t*)dtgt.p, 0, 0, (const long long*)doff.p,
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
