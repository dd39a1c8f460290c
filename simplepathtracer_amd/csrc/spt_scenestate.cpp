// spt_scenestate.cpp -- the scene state of a context (spt_host.h SceneState):
// the setters of scene, camera, params and traversal shape, spt_update_scene, the fold's colour
// table, and the host-only checks of what they build.  Two things reach the device from here,
// each by one path: traversal tables, built or refit (put_tables), and primary-ray candidate
// lists, the host builder's or the device's (update_lists).
//
// Synchronisation: a call ends a resident service session first (a device-wide wait would
// wait for it); the device is idle before a traversal table is written; this context's renders
// and feature calls are done before a list is, and the list kernel has finished before the
// call returns, so no launch in flight on any stream reads a half-written table.
#include "spt_host.h"

namespace spt_api {

namespace {

static_assert(kPrimPlanDevice == SPT_UPDATE_LISTS_DEVICE && kPrimPlanCamera == SPT_UPDATE_LISTS_CAMERA &&
                  kPrimPlanSlots == SPT_UPDATE_LISTS_SLOTS,
              "spt_primplan.h states the reasons of spt_hip.h");

using PrimKey = SceneState::PrimKey;

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// Halvings after which every finite albedo component a of the scene, as the diffuse code
// rebuilds it (a * 0.5f, then * 0.5f per further bounce: spt_kernels.hip halve_n), is 0;
// at most kCodeSat.  Saturating j there changes no colour (diffuse_code).
uint32_t halvings_to_zero(const std::vector<float4> &shade)
{
    uint32_t jz = 0;
    for (const float4 &s : shade)
        for (float a : {s.x, s.y, s.z}) {
            if (!std::isfinite(a)) continue;  // inf and NaN stay themselves
            volatile float x = a * 0.5f;
            uint32_t j = 0;
            while (x != 0.f && j < spt::kCodeSat) {
                x = x * 0.5f;
                ++j;
            }
            jz = std::max(jz, j);
        }
    return jz;
}

// ---- traversal tables ---------------------------------------------------------------------

// The tables of a scene in the shape (cluster size, branching) asks for, either of them
// possibly on auto: by default a 4-ary (3-ary above 512 spheres) tree of boxes over 8-sphere
// clusters (config 2: 14 650 Msamples/s against 13 950 for round 1's flat list of 4-sphere
// clusters under bounding spheres); the flat list remains selectable
// (spt_set_cluster_tree(ctx, 0)).  Scenes of <= 32 spheres are tested brute force
// (build_accel).  The contexts and the host-only checks build through here.
spt::AccelTables build_tables(const float *centers4, const float *radii, uint32_t n, uint32_t cluster_k, uint32_t branching)
{
    const bool tree = branching == SPT_TREE_AUTO ? true : branching >= 2;
    const uint32_t k = cluster_k != SPT_CLUSTER_AUTO ? cluster_k : tree ? spt::kClusterSlots : spt::kFlatLeafSlots;
    // auto: 4 children per node; 3 for large scenes, whose trees the LDS kernel walks
    // lane by lane (config 5: 107 ms per frame against 110 for 4)
    const uint32_t b = tree ? (branching == SPT_TREE_AUTO ? (n > 512 ? 3u : 4u) : branching) : 0u;
    const uint32_t leaf_slots = !tree && k <= spt::kFlatLeafSlots ? spt::kFlatLeafSlots : spt::kClusterSlots;
    return spt::build_accel(centers4, radii, n, k, spt::render_group_size(), b, leaf_slots);
}

// The one way traversal tables reach the device.  built: t is a fresh build for the context's
// scene and every array goes up; else ctx's own tables were refit in place, and slot centres,
// node records and pretest constants go up (shading tables, orig and the slot order stand).
// The view the kernels take is composed here and nowhere else.  A build that fails before its
// last upload leaves ctx->scene.tables, the view and the generations as they were.
int put_tables(spt_ctx *ctx, spt::AccelTables &t, bool built)
{
    SceneState &s = ctx->scene;
    std::vector<float4> shade;
    std::vector<uint32_t> mat;
    uint32_t jz = ctx->code_jz;
    if (built) {
        // a diffuse sample's code is 2 + j * slots + slot (diffuse_code); check_ready checks
        // that the scene's codes fit at the frame's depth
        jz = halvings_to_zero(s.h_shade);
        if (!spt::code_layout_fits(t.slots.size(), 0))
            return fail(ctx, SPT_ERR_ARG, "%zu sphere slots exceed the sample code space", t.slots.size());
        // shading tables in slot order: the kernel keeps the winner's slot, not its index
        shade.assign(t.slots.size(), make_float4(0.f, 0.f, 0.f, 0.f));
        mat.assign(t.slots.size(), SPT_SKYBOX);
        for (size_t j = 0; j < t.slots.size(); ++j)
            if (t.orig[j] != 0xFFFFFFFFu) {
                shade[j] = s.h_shade[t.orig[j]];
                mat[j] = s.h_mat[t.orig[j]];
            }
    }
    // every stream: host calls and caller-stream renders may still read the tables
    HIP_TRY(ctx, hipDeviceSynchronize());
    int rc = upload(ctx, &s.d_slots, &s.slots_cap, t.slots);
    if (!rc && built) rc = upload(ctx, &s.d_shade, &s.shade_cap, shade);
    if (!rc && built) rc = upload(ctx, &s.d_mat, &s.mat_cap, mat);
    if (!rc && built) rc = upload(ctx, &s.d_orig, &s.orig_cap, t.orig);
    if (!rc) rc = upload(ctx, &s.d_nodes, &s.nodes_cap, t.nodes);
    if (!rc) rc = upload(ctx, &s.d_kpre, &s.kpre_cap, t.kpre);
    if (rc) return rc;
    if (built) s.tables = std::move(t);
    const spt::AccelTables &now = s.tables;
    ctx->accel = spt::AccelView{s.d_slots, s.d_orig, s.d_nodes, now.always_groups, now.n_nodes,
                                now.n_nodes > now.leaves ? 1u : 0u, now.leaf_slots, s.d_kpre, now.pre_cm};
    ctx->code_stride = (uint32_t)std::max<size_t>(now.slots.size(), 1);
    ctx->code_jz = jz;
    // the candidate lists follow either (PrimKey); the fold's colour table a build only
    ++(built ? s.accel_gen : s.refit_gen);
    return SPT_OK;
}

// Build the tables of the context's scene (its host copy) in the context's shape.
int rebuild_accel(spt_ctx *ctx)
{
    SceneState &s = ctx->scene;
    const auto t0 = std::chrono::steady_clock::now();
    spt::AccelTables t = build_tables(s.h_centers.data(), s.h_radii.data(), ctx->n, ctx->cluster_k, ctx->tree_branching);
    const std::string bad = spt::validate_accel(t, s.h_centers.data(), s.h_radii.data(), ctx->n);
    if (!bad.empty()) return fail(ctx, SPT_ERR_STATE, "traversal tables invalid: %s", bad.c_str());
    if (int rc = put_tables(ctx, t, true)) return rc;
    s.accel_build_s = seconds_since(t0);
    return SPT_OK;
}

// ---- candidate lists ------------------------------------------------------------------------

// Lists are kept for the current state (none for trees walked lane by lane, which have no
// primary batches: casting their freshly started paths against the lists cut config 5's node
// visits per ray 17.1 -> 12.7 but not its walk iterations or time).
bool prim_wanted(const spt_ctx *ctx)
{
    return ctx->prim_enabled && ctx->scene_set && ctx->cam_set && ctx->params_set && !spt::lane_walk_tree(ctx->accel);
}

// what lists built now would be built for
PrimKey prim_key_now(const spt_ctx *ctx)
{
    PrimKey key{};
    for (int i = 0; i < 12; ++i) key.view[i] = ctx->cam.view[i];
    for (int i = 0; i < 3; ++i) key.eye[i] = ctx->cam.eye[i];
    key.W = ctx->W;
    key.H = ctx->H;
    key.prim_max = ctx->prim_max;
    key.accel_gen = ctx->scene.accel_gen;
    key.refit_gen = ctx->scene.refit_gen;
    key.valid = true;
    return key;
}

// no lists: every primary batch walks the tree
void prim_drop(spt_ctx *ctx)
{
    SceneState &s = ctx->scene;
    ctx->prim = spt::PrimLists{};
    s.prim_blocks = s.prim_entries = s.prim_slots_n = 0;
    s.prim_key = PrimKey{};
}

// The one way candidate lists reach the device: those of the context's current tables, camera
// and frame.  info null: a setter's call, which never builds on the device (its lists are the
// host builder's packed runs); else spt_update_scene's, with the info to fill.
int update_lists(spt_ctx *ctx, spt_update_info *info)
{
    SceneState &s = ctx->scene;
    const bool device_allowed = info != nullptr;
    spt_update_info unused{};
    if (!info) info = &unused;
    auto done = [&](uint32_t reason) {
        info->lists_reason = reason;
        info->list_blocks = s.prim_blocks;
        info->list_entries = s.prim_entries;
        return SPT_OK;
    };
    // wanted at all?  If not, nothing is kept, the key neither
    if (!prim_wanted(ctx)) {
        prim_drop(ctx);
        return done(SPT_UPDATE_LISTS_OFF);
    }
    // the lists depend on the tables, the camera and the frame size only
    const PrimKey key = prim_key_now(ctx);
    if (key.same(s.prim_key)) return done(SPT_UPDATE_LISTS_UNCHANGED);
    // who builds: where the host builder turns the lists off, it decides (spt_primplan.h)
    const spt::AccelTables &t = s.tables;
    const uint32_t pad = device_allowed ? spt::prim_pad_slot(t) : spt::kPrimWalk;
    const PrimPlan plan = device_allowed ? prim_plan(t.slots.size(), ctx->W, ctx->H, ctx->prim_max, ctx->prim_dev_slots,
                                                     spt::prim_camera_usable(ctx->cam), pad != spt::kPrimWalk)
                                         : PrimPlan{};
    // the old lists are gone whatever happens next
    prim_drop(ctx);
    // the host builder touches nothing on the device: it runs beside the renders in flight
    spt::PrimListTables pl;
    if (!plan.device) pl = spt::build_prim_lists(t, ctx->cam, ctx->W, ctx->H, ctx->prim_max);
    // this context's renders and feature calls in flight may still read the previous lists
    if (plan.device || pl.on)
        if (int rc = wait_own_renders(ctx)) return rc;
    // the lists on the device: the kernel's runs at fixed strides, or the host's packed ones
    uint32_t blocks = 0, entries = 0, slots_n = 0, bw = plan.bw;
    double build_s = pl.seconds;
    if (plan.device) {
        int rc = ensure(ctx, &s.d_prim_b8, &s.prim_b8_cap, plan.nb8);
        if (!rc) rc = ensure(ctx, &s.d_prim_b4, &s.prim_b4_cap, plan.nb4);
        if (!rc) rc = ensure(ctx, &s.d_prim_slots, &s.prim_slots_cap, (size_t)std::max<uint64_t>(plan.total, 4));
        if (rc) return rc;
        if (!s.d_prim_totals) HIP_TRY(ctx, hipMalloc((void **)&s.d_prim_totals, 2 * sizeof(uint32_t)));
        for (hipEvent_t &e : s.upd_ev)
            if (!e) HIP_TRY(ctx, hipEventCreate(&e));
        const spt::PrimBuildArgs a{s.d_slots, (uint32_t)t.slots.size(), pad, ctx->cam, ctx->W, ctx->H, ctx->prim_max,
                                   plan.stride, plan.bw, plan.nb8, s.d_prim_b8, s.d_prim_b4, s.d_prim_slots, s.d_prim_totals};
        HIP_TRY(ctx, hipMemsetAsync(s.d_prim_totals, 0, 2 * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipEventRecord(s.upd_ev[0], ctx->stream));
        HIP_TRY(ctx, spt::launch_prim_lists(a, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(s.upd_ev[1], ctx->stream));
        // like the host path's blocking uploads: the lists are whole before any launch reads them
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        uint32_t totals[2] = {0, 0};  // 8x8 blocks with a list, entries
        HIP_TRY(ctx, hipMemcpy(totals, s.d_prim_totals, sizeof totals, hipMemcpyDeviceToHost));
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, s.upd_ev[0], s.upd_ev[1]));
        blocks = totals[0];
        entries = totals[1];
        slots_n = (uint32_t)plan.total;
        build_s = ms * 1e-3;
        info->lists_ms = ms;
        info->lists_on_device = 1;
    } else if (pl.on) {
        int rc = upload(ctx, &s.d_prim_b8, &s.prim_b8_cap, pl.b8);
        if (!rc) rc = upload(ctx, &s.d_prim_b4, &s.prim_b4_cap, pl.b4);
        if (!rc) rc = upload(ctx, &s.d_prim_slots, &s.prim_slots_cap, pl.slots);
        if (rc) return rc;
        for (const uint2 &b : pl.b8) blocks += b.y != spt::kPrimWalk ? 1u : 0u;
        entries = slots_n = (uint32_t)pl.slots.size();
        bw = pl.bw;
    }
    // install, here only; with the key also where the host builder answered "off" (asked once)
    if (plan.device || pl.on) ctx->prim = spt::PrimLists{s.d_prim_b8, s.d_prim_b4, s.d_prim_slots, bw, 1u};
    s.prim_blocks = blocks;
    s.prim_entries = entries;
    s.prim_slots_n = slots_n;
    s.prim_key = key;
    s.prim_builds++;
    s.prim_build_s = build_s;
    return done(plan.device ? SPT_UPDATE_LISTS_DEVICE : plan.reason);
}

// ---- small rules ----------------------------------------------------------------------------

// view as spt_set_camera takes it
int check_view(spt_ctx *ctx, const float view[16])
{
    for (int j = 12; j < 16; ++j)
        if (view[j] != 0.0f)
            return fail(ctx, SPT_ERR_ARG, "viewMatrix row 3 must be zero (CreateCameraBasisMatrix, Math.hpp:204-208)");
    return SPT_OK;
}

// Lists pl of tables t in the output format of spt_prim_lists_check and spt_prim_lists_read
int lists_out(spt_ctx *ctx, const spt::PrimListTables &pl, const spt::AccelTables &t, uint32_t *blocks8, uint32_t *blocks4,
              uint32_t *slot_ids, uint32_t *slot_orig, uint32_t cap, uint32_t *counts)
{
    counts[0] = (uint32_t)pl.slots.size();
    counts[1] = (uint32_t)t.slots.size();
    counts[2] = pl.bw;
    counts[3] = pl.on ? 1u : 0u;
    if ((slot_ids && cap < pl.slots.size()) || (slot_orig && cap < t.slots.size()))
        return fail(ctx, SPT_ERR_ARG, "capacity %u < %zu list entries / %zu slots", cap, pl.slots.size(), t.slots.size());
    // {first, count} per block: a uint2 is its two words
    if (blocks8) std::copy_n((const uint32_t *)pl.b8.data(), 2 * pl.b8.size(), blocks8);
    if (blocks4) std::copy_n((const uint32_t *)pl.b4.data(), 2 * pl.b4.size(), blocks4);
    if (slot_ids) std::copy(pl.slots.begin(), pl.slots.end(), slot_ids);
    if (slot_orig) std::copy(t.orig.begin(), t.orig.end(), slot_orig);
    return SPT_OK;
}

// What every call that changes the state of member c does first, under c's lock
int begin_change(spt_ctx *c)
{
    if (int rc = svc_end(c)) return rc;  // the session holds the state the call changes
    c->gen++;                            // a read-ahead frame of the old state is stale
    return SPT_OK;
}

// spt_set_cluster_size (tree false) and spt_set_cluster_tree of one member
int set_shape(spt_ctx *ctx, bool tree, uint32_t v)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = begin_change(ctx)) return rc;
    if (!tree && v > spt::kClusterSlots && v != SPT_CLUSTER_AUTO)
        return fail(ctx, SPT_ERR_ARG, "cluster size %u > %u", v, spt::kClusterSlots);
    if (tree && (v == 1 || (v > 64 && v != SPT_TREE_AUTO)))
        return fail(ctx, SPT_ERR_ARG, "tree branching %u not in {0, 2..64, SPT_TREE_AUTO}", v);
    (tree ? ctx->tree_branching : ctx->cluster_k) = v;
    if (!ctx->scene_set) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = rebuild_accel(ctx);
    return rc ? rc : update_lists(ctx, nullptr);
}

}  // namespace

// ---- the fold's colour table ----------------------------------------------------------------
// The table (spt_codes.h) for the current scene tables and depth: one entry per diffuse code,
// filled on the device by the arithmetic decode (ctab_fill_kernel).  It depends on the shading
// table, the slot order (code_stride) and jmax only, which the scene, cluster and params
// setters change: they leave the table stale (ctab_valid), and the first launched render after
// them (render_impl) calls rebuild_ctab; nothing is done while the table stands, and a refit
// leaves it standing.  Like the scene uploads it waits for the device on both sides: launches
// in flight on any stream may read the old table, and the launches enqueued after it on any
// stream read the new one.
bool ctab_valid(const spt_ctx *ctx)
{
    const SceneState &s = ctx->scene;
    return s.ctab_n != 0 && s.ctab_gen == s.accel_gen && s.ctab_jmax == code_jmax(ctx);
}

int rebuild_ctab(spt_ctx *ctx)
{
    SceneState &s = ctx->scene;
    const uint32_t jmax = code_jmax(ctx);
    if (s.ctab_gen == s.accel_gen && s.ctab_jmax == jmax) return SPT_OK;
    if (int rc = svc_end(ctx)) return rc;  // a resident session would hold the synchronisation
    s.ctab_n = 0;
    s.ctab_gen = s.accel_gen;
    s.ctab_jmax = jmax;
    if (!spt::ctab_fits(ctx->code_stride, jmax) || !spt::code_layout_fits(ctx->code_stride, jmax)) return SPT_OK;
    const uint32_t n = (uint32_t)spt::ctab_entries(ctx->code_stride, jmax);
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (int rc = ensure(ctx, &s.d_ctab, &s.ctab_cap, n)) return rc;
    spt::FoldArgs fa = fold_args(ctx, nullptr, 1u);
    HIP_TRY(ctx, spt::launch_ctab_fill(fa, s.d_ctab, n, nullptr));
    HIP_TRY(ctx, hipStreamSynchronize(nullptr));
    s.ctab_n = n;
    return SPT_OK;
}

}  // namespace spt_api

extern "C" {

// The setters apply to the context and to every member device of a multi-device context, each
// under its own hipSetDevice (for_members refuses a null context and a progress callback).

int spt_set_scene(spt_ctx *ctx, const float *centers4, const float *radii, const float *colors4,
                  const uint8_t *materials, const float *fuzz, uint32_t n)
{
    return for_members(ctx, [&](spt_ctx *c) -> int {
        std::lock_guard<std::mutex> lk(c->mu);
        if (int rc = begin_change(c)) return rc;
        if (n > 0 && (!centers4 || !radii || !colors4 || !materials || !fuzz))
            return fail(c, SPT_ERR_ARG, "null scene array");
        HIP_TRY(c, hipSetDevice(c->device));
        SceneState &s = c->scene;
        s.h_shade.resize(n);
        s.h_mat.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            s.h_shade[i] = make_float4(colors4[4 * i], colors4[4 * i + 1], colors4[4 * i + 2], fuzz[i]);
            s.h_mat[i] = materials[i];
        }
        s.h_centers.assign(centers4, centers4 + 4 * (size_t)n);
        s.h_radii.assign(radii, radii + n);
        c->n = n;
        if (int rc = rebuild_accel(c)) return rc;
        c->scene_set = true;
        return update_lists(c, nullptr);
    });
}

int spt_set_camera(spt_ctx *ctx, const float view[16], const float eye[4], const float sky[4])
{
    return for_members(ctx, [&](spt_ctx *c) -> int {
        std::lock_guard<std::mutex> lk(c->mu);
        if (int rc = begin_change(c)) return rc;
        if (!view || !eye || !sky) return fail(c, SPT_ERR_ARG, "null camera array");
        if (int rc = check_view(c, view)) return rc;
        for (int j = 0; j < 12; ++j) c->cam.view[j] = view[j];
        for (int j = 0; j < 3; ++j) {
            c->cam.eye[j] = eye[j];
            c->cam.sky[j] = sky[j];
        }
        c->cam_set = true;
        HIP_TRY(c, hipSetDevice(c->device));
        return update_lists(c, nullptr);
    });
}

int spt_set_params(spt_ctx *ctx, uint32_t width, uint32_t height, uint32_t spp, uint32_t bounces, uint64_t seed)
{
    return for_members(ctx, [&](spt_ctx *c) -> int {
        std::unique_lock<std::mutex> lk(c->mu);
        if (int rc = begin_change(c)) return rc;
        if (width == 0 || height == 0) return fail(c, SPT_ERR_ARG, "empty frame %ux%u", width, height);
        if ((uint64_t)width * height * 3 > 0xFFFFFFFFull)
            return fail(c, SPT_ERR_ARG, "frame %ux%u overflows the reference's uint32 g_size", width, height);
        if (spp == 0) return fail(c, SPT_ERR_ARG, "spp must be >= 1 (1.f/0 samples)");
        if (bounces == 0) return fail(c, SPT_ERR_ARG, "bounces must be >= 1 (--bounceCount never reaches 0)");
        c->W = width;
        c->H = height;
        c->spp = spp;
        c->bounces = bounces;
        c->seed = seed;
        c->params_set = true;
        HIP_TRY(c, hipSetDevice(c->device));
        const int rc = update_lists(c, nullptr);
        // the drop-in (spt_prepare_dropin) renders its first frame through the tiling read-ahead:
        // its page-locked frame now, with the setup, not in that frame.  Last, once the context
        // is whole again, as it may wait unlocked for serves in progress; best effort: else at
        // the first tile-shaped call
        if (c->spec.st.arm_first() && c->readahead) (void)spec_frame_bytes(c, lk, (size_t)width * height * 3);
        return rc;
    });
}

int spt_set_cluster_size(spt_ctx *ctx, uint32_t k)
{
    return for_members(ctx, [&](spt_ctx *c) { return set_shape(c, false, k); });
}

int spt_set_cluster_tree(spt_ctx *ctx, uint32_t branching)
{
    return for_members(ctx, [&](spt_ctx *c) { return set_shape(c, true, branching); });
}

int spt_update_scene(spt_ctx *ctx, const float *centers4, const float view[16], const float eye[4], spt_update_info *info)
{
    spt_update_info *out = info;  // member 0's; the other members' go nowhere
    return for_members(ctx, [&](spt_ctx *c) -> int {
        std::lock_guard<std::mutex> lk(c->mu);
        if (int rc = begin_change(c)) return rc;
        SceneState &s = c->scene;
        spt_update_info local{};
        spt_update_info *inf = out ? out : &local;
        out = nullptr;
        *inf = spt_update_info{};
        if ((view == nullptr) != (eye == nullptr)) return fail(c, SPT_ERR_ARG, "view and eye come together");
        if (view)
            if (int rc = check_view(c, view)) return rc;
        if (!c->scene_set) return fail(c, SPT_ERR_STATE, "spt_update_scene before spt_set_scene");
        if (view && !c->cam_set)
            return fail(c, SPT_ERR_STATE, "spt_update_scene moves a camera spt_set_camera has set (the sky is its)");
        HIP_TRY(c, hipSetDevice(c->device));
        if (centers4 && c->n > 0) {
            const auto t0 = std::chrono::steady_clock::now();
            // refit_accel checks before it writes: refused, the tables are as they were.  Its result is
            // not validated here (validate_accel gathers members per node; spt_accel_refit_check runs it)
            const std::string bad = spt::refit_accel(s.tables, centers4, s.h_radii.data(), c->n);
            if (!bad.empty()) return fail(c, SPT_ERR_ARG, "refit refused: %s", bad.c_str());
            // the host copy follows: a later spt_set_cluster_tree or _size rebuilds from the moved centres
            s.h_centers.assign(centers4, centers4 + 4 * (size_t)c->n);
            if (int rc = put_tables(c, s.tables, false)) return rc;
            inf->refit_ms = seconds_since(t0) * 1e3;
            inf->refit = 1;
        }
        if (view) {
            for (int j = 0; j < 12; ++j) c->cam.view[j] = view[j];
            for (int j = 0; j < 3; ++j) c->cam.eye[j] = eye[j];
        }
        return update_lists(c, inf);
    });
}

// ---- host-only checks -----------------------------------------------------------------------

int spt_accel_refit_check(const float *centers_a, const float *centers_b, const float *radii, uint32_t n, uint32_t cluster_k,
                          uint32_t branching, int refit, uint32_t *counts, float *slots4, uint32_t *orig, float *kpre,
                          uint32_t *nodes, float *pre_cm, uint32_t cap_slots, uint32_t cap_nodes)
{
    if (n > 0 && (!centers_a || !radii || (refit && !centers_b))) return fail(nullptr, SPT_ERR_ARG, "null scene array");
    if (cluster_k > spt::kClusterSlots) return fail(nullptr, SPT_ERR_ARG, "cluster size %u > %u", cluster_k, spt::kClusterSlots);
    if (branching == 1) return fail(nullptr, SPT_ERR_ARG, "tree branching 1");
    spt::AccelTables t = build_tables(centers_a, radii, n, cluster_k, branching);
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

int spt_accel_check(const float *centers4, const float *radii, uint32_t n, uint32_t cluster_k, uint32_t branching,
                    uint32_t *out_nodes)
{
    uint32_t counts[4] = {};
    const int rc = spt_accel_refit_check(centers4, nullptr, radii, n, cluster_k, branching, 0, counts, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, 0, 0);
    if (!rc && out_nodes) *out_nodes = counts[2];
    return rc;
}

int spt_prim_lists_check(const float *centers4, const float *radii, uint32_t n, const float view[16], const float eye[4],
                         uint32_t width, uint32_t height, uint32_t max_count, uint32_t *blocks8, uint32_t *blocks4,
                         uint32_t *slot_ids, uint32_t *slot_orig, uint32_t cap, uint32_t *counts)
{
    if (n > 0 && (!centers4 || !radii)) return fail(nullptr, SPT_ERR_ARG, "null scene array");
    if (!view || !eye || !counts || width == 0 || height == 0) return fail(nullptr, SPT_ERR_ARG, "bad arguments");
    // the default traversal shape: both settings on auto
    const spt::AccelTables t = build_tables(centers4, radii, n, SPT_CLUSTER_AUTO, SPT_TREE_AUTO);
    spt::Camera cam{};
    for (int j = 0; j < 12; ++j) cam.view[j] = view[j];
    for (int j = 0; j < 3; ++j) cam.eye[j] = eye[j];
    const spt::PrimListTables pl = spt::build_prim_lists(t, cam, width, height, max_count);
    return lists_out(nullptr, pl, t, blocks8, blocks4, slot_ids, slot_orig, cap, counts);
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
    const SceneState &s = ctx->scene;
    const uint32_t bw = (ctx->W + 7) / 8;
    const size_t nb8 = (size_t)bw * ((ctx->H + 7) / 8), nb4 = (size_t)bw * ((ctx->H + 3) / 4);
    spt::PrimListTables pl;
    if (which == 1) pl = spt::build_prim_lists(s.tables, ctx->cam, ctx->W, ctx->H, ctx->prim_max);
    else pl.on = ctx->prim.on;
    pl.bw = bw;
    pl.b8.resize(nb8, make_uint2(0, spt::kPrimWalk));
    pl.b4.resize(nb4, make_uint2(0, spt::kPrimWalk));
    if (which == 0 && pl.on) {
        pl.slots.resize(s.prim_slots_n);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        // the lists were whole when their build returned; nothing writes them until the next
        HIP_TRY(ctx, hipMemcpy(pl.b8.data(), s.d_prim_b8, nb8 * sizeof(uint2), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(pl.b4.data(), s.d_prim_b4, nb4 * sizeof(uint2), hipMemcpyDeviceToHost));
        if (!pl.slots.empty())
            HIP_TRY(ctx, hipMemcpy(pl.slots.data(), s.d_prim_slots, pl.slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return lists_out(ctx, pl, s.tables, blocks8, blocks4, slot_ids, slot_orig, cap, counts);
}

}  // extern "C"
