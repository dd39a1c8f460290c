// spt_update.cpp -- scene updates (include/spt_hip.h "scene updates"):
// spt_update_scene moves the spheres and / or the camera of a context without the setters'
// host work.  The traversal tables are refit (spt_accel.cpp refit_accel: same shape, every
// bound recomputed with the builder's arithmetic) and uploaded; the primary-ray candidate
// lists are built by spt_primlists.hip on the device, or by the host builder where the
// kernel does not apply.  Everything a render, query or feature call computes afterwards is
// what it computes after spt_set_scene + spt_set_camera: the cull conditions use only the
// containment of a node's members, the list cast only that a ray's winner is in its list.
//
// Synchronisation is the setters': the device is idle before a traversal table is written
// (rebuild_accel), this context's renders and feature calls are done before a list is
// (rebuild_prim), and the list kernel has finished before the call returns, so no launch in
// flight on any stream reads a half-written table.
#include "spt_host.h"

namespace spt_api {

namespace {

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Refit ctx->tables to the new centres and upload what changed: slot centres, node records,
// pretest constants (shading tables, orig and the slot order stand).
int refit_scene(spt_ctx *ctx, const float *centers4, spt_update_info *info)
{
    const auto t0 = std::chrono::steady_clock::now();
    // refit_accel checks before it writes: on an error the tables are as they were
    const std::string bad = spt::refit_accel(ctx->tables, centers4, ctx->h_radii.data(), ctx->n);
    if (!bad.empty()) return fail(ctx, SPT_ERR_ARG, "refit refused: %s", bad.c_str());
    ctx->h_centers.assign(centers4, centers4 + 4 * (size_t)ctx->n);
    ctx->refit_gen++;  // the candidate lists follow (PrimKey); the fold's colour table does not
    // not validated here (validate_accel gathers members per node; spt_accel_refit_check runs it)
    const spt::AccelTables &t = ctx->tables;
    // every stream: host calls and caller-stream renders may still read the tables
    HIP_TRY(ctx, hipDeviceSynchronize());
    int rc = upload(ctx, &ctx->d_slots, &ctx->slots_cap, t.slots);
    if (!rc) rc = upload(ctx, &ctx->d_nodes, &ctx->nodes_cap, t.nodes);
    if (!rc) rc = upload(ctx, &ctx->d_kpre, &ctx->kpre_cap, t.kpre);
    if (rc) return rc;
    ctx->accel.slots = ctx->d_slots;
    ctx->accel.nodes = ctx->d_nodes;
    ctx->accel.kpre = ctx->d_kpre;
    ctx->accel.pre_cm = t.pre_cm;
    info->refit_ms = ms_since(t0);
    info->refit = 1;
    return SPT_OK;
}

// The candidate lists for the context's current tables, camera and frame: by the kernel
// where it applies, else as rebuild_prim builds (or drops) them.
int update_lists(spt_ctx *ctx, spt_update_info *info)
{
    auto host = [&](uint32_t reason) {
        info->lists_reason = reason;
        const int rc = rebuild_prim(ctx);
        info->list_blocks = ctx->prim_blocks;
        info->list_entries = ctx->prim_entries;
        return rc;
    };
    if (!prim_wanted(ctx)) return host(SPT_UPDATE_LISTS_OFF);
    const spt_ctx::PrimKey key = prim_key_now(ctx);
    if (key.same(ctx->prim_key)) {
        info->lists_reason = SPT_UPDATE_LISTS_UNCHANGED;
        info->list_blocks = ctx->prim_blocks;
        info->list_entries = ctx->prim_entries;
        return SPT_OK;
    }
    // where the host builder turns the lists off, it decides (build_prim_lists)
    const spt::AccelTables &t = ctx->tables;
    const uint32_t W = ctx->W, H = ctx->H;
    const uint32_t pad = spt::prim_pad_slot(t);
    if (W > 0xFFFFu || H > 0xFFFFu || !spt::prim_camera_usable(ctx->cam) || pad == spt::kPrimWalk)
        return host(SPT_UPDATE_LISTS_CAMERA);
    const uint32_t bw = (W + 7) / 8, nb8 = bw * ((H + 7) / 8), nb4 = bw * ((H + 3) / 4);
    const uint32_t stride = (ctx->prim_max + 3u) & ~3u;
    const uint64_t total = ((uint64_t)nb8 + nb4) * stride;
    // the kernel's LDS list holds kPrimDevSlots slots; a run's first entry is a uint32
    if (t.slots.size() > ctx->prim_dev_slots || total > 0xFFFFFFFFull) return host(SPT_UPDATE_LISTS_SLOTS);

    prim_drop(ctx);
    // this context's renders in flight may still read the previous lists
    if (int rc = wait_own_renders(ctx)) return rc;
    int rc = ensure(ctx, &ctx->d_prim_b8, &ctx->prim_b8_cap, nb8);
    if (!rc) rc = ensure(ctx, &ctx->d_prim_b4, &ctx->prim_b4_cap, nb4);
    if (!rc) rc = ensure(ctx, &ctx->d_prim_slots, &ctx->prim_slots_cap, (size_t)std::max<uint64_t>(total, 4));
    if (rc) return rc;
    if (!ctx->d_prim_totals) HIP_TRY(ctx, hipMalloc((void **)&ctx->d_prim_totals, 2 * sizeof(uint32_t)));
    for (hipEvent_t &e : ctx->upd_ev)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    spt::PrimBuildArgs a{};
    a.slots = ctx->d_slots;
    a.n_slots = (uint32_t)t.slots.size();
    a.pad = pad;
    a.cam = ctx->cam;
    a.W = W;
    a.H = H;
    a.prim_max = ctx->prim_max;
    a.stride = stride;
    a.bw = bw;
    a.nb8 = nb8;
    a.b8 = ctx->d_prim_b8;
    a.b4 = ctx->d_prim_b4;
    a.out = ctx->d_prim_slots;
    a.totals = ctx->d_prim_totals;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_prim_totals, 0, 2 * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->upd_ev[0], ctx->stream));
    HIP_TRY(ctx, spt::launch_prim_lists(a, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->upd_ev[1], ctx->stream));
    // like the host path's blocking uploads: the lists are whole before any launch reads them
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t totals[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpy(totals, ctx->d_prim_totals, sizeof totals, hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->upd_ev[0], ctx->upd_ev[1]));
    ctx->prim = spt::PrimLists{ctx->d_prim_b8, ctx->d_prim_b4, ctx->d_prim_slots, bw, 1u};
    ctx->prim_blocks = totals[0];
    ctx->prim_entries = totals[1];
    ctx->prim_slots_n = (uint32_t)total;
    ctx->prim_key = key;
    ctx->prim_builds++;
    ctx->prim_build_s = ms * 1e-3;
    info->lists_ms = ms;
    info->lists_on_device = 1;
    info->lists_reason = SPT_UPDATE_LISTS_DEVICE;
    info->list_blocks = totals[0];
    info->list_entries = totals[1];
    return SPT_OK;
}

}  // namespace

int spt_update_scene_one(spt_ctx *ctx, const float *centers4, const float view[16], const float eye[4],
                         spt_update_info *info)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc_ = svc_end(ctx)) return rc_;  // the session holds the state this call changes
    ctx->gen++;                              // a read-ahead frame of the old state is stale
    spt_update_info local{};
    if (!info) info = &local;
    *info = spt_update_info{};
    if ((view == nullptr) != (eye == nullptr)) return fail(ctx, SPT_ERR_ARG, "view and eye come together");
    for (int j = 12; view && j < 16; ++j)
        if (view[j] != 0.0f)
            return fail(ctx, SPT_ERR_ARG, "viewMatrix row 3 must be zero (CreateCameraBasisMatrix, Math.hpp:204-208)");
    if (!ctx->scene_set) return fail(ctx, SPT_ERR_STATE, "spt_update_scene before spt_set_scene");
    if (view && !ctx->cam_set) return fail(ctx, SPT_ERR_STATE, "spt_update_scene moves a camera spt_set_camera has set (the sky is its)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (centers4 && ctx->n > 0)
        if (int rc = refit_scene(ctx, centers4, info)) return rc;
    if (view) {
        for (int j = 0; j < 12; ++j) ctx->cam.view[j] = view[j];
        for (int j = 0; j < 3; ++j) ctx->cam.eye[j] = eye[j];
    }
    return update_lists(ctx, info);
}

}  // namespace spt_api

extern "C" {

int spt_update_scene(spt_ctx *ctx, const float *centers4, const float view[16], const float eye[4], spt_update_info *info)
{
    bool first = true;
    return for_members(ctx, [&](spt_ctx *c) {
        // info: member 0's
        const int rc = spt_update_scene_one(c, centers4, view, eye, first ? info : nullptr);
        first = false;
        return rc;
    });
}

int spt_accel_refit_check(const float *centers_a, const float *centers_b, const float *radii, uint32_t n, uint32_t cluster_k,
                          uint32_t branching, int refit, uint32_t *counts, float *slots4, uint32_t *orig, float *kpre,
                          uint32_t *nodes, float *pre_cm, uint32_t cap_slots, uint32_t cap_nodes)
{
    if (n > 0 && (!centers_a || !radii || (refit && !centers_b))) return fail(nullptr, SPT_ERR_ARG, "null scene array");
    if (cluster_k > spt::kClusterSlots) return fail(nullptr, SPT_ERR_ARG, "cluster size %u > %u", cluster_k, spt::kClusterSlots);
    if (branching == 1) return fail(nullptr, SPT_ERR_ARG, "tree branching 1");
    const uint32_t leaf = branching == 0 && cluster_k <= spt::kFlatLeafSlots ? spt::kFlatLeafSlots : spt::kClusterSlots;
    spt::AccelTables t = spt::build_accel(centers_a, radii, n, cluster_k, spt::render_group_size(), branching, leaf);
    const float *now = centers_a;
    if (refit) {
        const std::string bad = spt::refit_accel(t, centers_b, radii, n);
        if (!bad.empty()) return fail(nullptr, SPT_ERR_ARG, "refit refused: %s", bad.c_str());
        now = centers_b;
    }
    const std::string inv = spt::validate_accel(t, now, radii, n);
    if (!inv.empty()) return fail(nullptr, SPT_ERR_STATE, "traversal tables invalid: %s", inv.c_str());
    if (counts) {
        counts[0] = (uint32_t)t.slots.size();
        counts[1] = (uint32_t)t.nodes.size();
        counts[2] = t.n_nodes;
        counts[3] = t.leaves;
    }
    if (((slots4 || orig || kpre) && cap_slots < t.slots.size()) || (nodes && cap_nodes < t.nodes.size()))
        return fail(nullptr, SPT_ERR_ARG, "capacity %u slots / %u records < %zu / %zu", cap_slots, cap_nodes, t.slots.size(),
                    t.nodes.size());
    if (slots4) std::memcpy(slots4, t.slots.data(), t.slots.size() * sizeof(float4));
    if (orig) std::memcpy(orig, t.orig.data(), t.orig.size() * sizeof(uint32_t));
    if (kpre) std::memcpy(kpre, t.kpre.data(), t.kpre.size() * sizeof(float));
    if (nodes) std::memcpy(nodes, t.nodes.data(), t.nodes.size() * sizeof(spt::AccelNode));
    if (pre_cm) *pre_cm = t.pre_cm;
    return SPT_OK;
}

int spt_prim_lists_read(spt_ctx *ctx, int which, uint32_t *blocks8, uint32_t *blocks4, uint32_t *slot_ids,
                        uint32_t *slot_orig, uint32_t cap, uint32_t *counts)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    if (int rc = check_not_in_callback(ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!counts || (which != 0 && which != 1)) return fail(ctx, SPT_ERR_ARG, "bad arguments");
    if (!ctx->scene_set || !ctx->cam_set || !ctx->params_set)
        return fail(ctx, SPT_ERR_STATE, "scene, camera and params must be set first");
    const spt::AccelTables &t = ctx->tables;
    const uint32_t bw = (ctx->W + 7) / 8;
    const size_t nb8 = (size_t)bw * ((ctx->H + 7) / 8), nb4 = (size_t)bw * ((ctx->H + 3) / 4);
    std::vector<uint2> b8, b4;
    std::vector<uint32_t> ids;
    bool on = false;
    if (which == 1) {
        spt::PrimListTables pl = spt::build_prim_lists(t, ctx->cam, ctx->W, ctx->H, ctx->prim_max);
        on = pl.on;
        b8 = std::move(pl.b8);
        b4 = std::move(pl.b4);
        ids = std::move(pl.slots);
    } else if (ctx->prim.on) {
        on = true;
        b8.resize(nb8);
        b4.resize(nb4);
        ids.resize(ctx->prim_slots_n);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        // the lists were whole when their build returned; nothing writes them until the next
        HIP_TRY(ctx, hipMemcpy(b8.data(), ctx->d_prim_b8, nb8 * sizeof(uint2), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(b4.data(), ctx->d_prim_b4, nb4 * sizeof(uint2), hipMemcpyDeviceToHost));
        if (!ids.empty())
            HIP_TRY(ctx, hipMemcpy(ids.data(), ctx->d_prim_slots, ids.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    b8.resize(nb8, make_uint2(0, spt::kPrimWalk));
    b4.resize(nb4, make_uint2(0, spt::kPrimWalk));
    counts[0] = (uint32_t)ids.size();
    counts[1] = (uint32_t)t.slots.size();
    counts[2] = bw;
    counts[3] = on ? 1u : 0u;
    if ((slot_ids && cap < ids.size()) || (slot_orig && cap < t.slots.size()))
        return fail(ctx, SPT_ERR_ARG, "capacity %u < %zu list entries / %zu slots", cap, ids.size(), t.slots.size());
    for (size_t i = 0; blocks8 && i < nb8; ++i) {
        blocks8[2 * i] = b8[i].x;
        blocks8[2 * i + 1] = b8[i].y;
    }
    for (size_t i = 0; blocks4 && i < nb4; ++i) {
        blocks4[2 * i] = b4[i].x;
        blocks4[2 * i + 1] = b4[i].y;
    }
    if (slot_ids) std::copy(ids.begin(), ids.end(), slot_ids);
    if (slot_orig) std::copy(t.orig.begin(), t.orig.end(), slot_orig);
    return SPT_OK;
}

}  // extern "C"
