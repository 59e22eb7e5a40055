// api_upload.hip -- flx_upload_scene (reference wire arrays -> the traversal layout: inner-node records, leaf runs, shading records, the 4-wide
// quantised tree) and flx_upload_envmap (alias records, the per-texel NEE table).  Both build the new set first and switch over only on success.
#include "flx_ctx.h"
#include "flx_wide.h"
#include "flx_refit.h"
#include "flx_mesh_light.h"
#include "flx_trace.h"
#include "flx_trace4.h"
#include <cmath>
#include <cstring>

// a failed copy releases what this upload has allocated so far (`bail` of the calling function)
#define UPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { c->err = std::string(#expr) + ": " + hipGetErrorString(e_); return bail(); } } while (0)

extern "C" {

// ---- scene upload: reference wire arrays -> traversal layout -------------------------------
int flx_upload_scene(flx_ctx *c, const void *trisv, size_t ntris, const uint32_t *indices, size_t nidx,
                     const void *nodesv, size_t nnodes, const void *materials, size_t nmat,
                     const void *texdesc, size_t ntex, const uint8_t *texdata, size_t texbytes)
{
    ENTER(c, CALL_OBSERVE);
    c->ad.state.dropped();                                // a list of active pixels belongs to the render of one scene (flx_mk_adaptive_clear)
    NEED(c, trisv && ntris && indices && nidx && nodesv && nnodes, "flx_upload_scene: empty scene");
    NEED(c, materials && nmat, "flx_upload_scene: at least the default material is required");
    HIPCHK(c, hipSetDevice(c->device));
    const flx_triangle *tris = (const flx_triangle *)trisv;
    const flx_node *nodes = (const flx_node *)nodesv;

    // 0. which BSDF types the fused logic+material pass inlines for this scene (logic.hip).  Inlining a type costs registers whether or not
    // a path of that type shows up, routing a type through its queue costs a second trip over the path state: measured on the three bench
    // scenes, a mostly-diffuse scene (kitchen 96 %, courtyard 65 % of the surface area) wants the diffuse step alone inline (+1..3 % Mrays/s
    // over the separate kernels, inlining everything +-0), a scene whose surfaces are mostly glossy / GGX (conference: 13 % diffuse) wants
    // them all (+11 %).  The reference specialises its kernels per scene too (-DBXDF_USE_*).  Option "fuse_set" overrides.
    {
        const flx_material *mats = (const flx_material *)materials;
        double areaAll = 0.0, areaDiffuse = 0.0;
        for (size_t i = 0; i < ntris; i++) {
            const flx_triangle &t = tris[i];
            const double ax = (double)t.v1.p.x - t.v0.p.x, ay = (double)t.v1.p.y - t.v0.p.y, az = (double)t.v1.p.z - t.v0.p.z;
            const double bx = (double)t.v2.p.x - t.v0.p.x, by = (double)t.v2.p.y - t.v0.p.y, bz = (double)t.v2.p.z - t.v0.p.z;
            const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            const double a = std::sqrt(cx * cx + cy * cy + cz * cz);
            areaAll += a;
            if (t.matId >= 0 && (size_t)t.matId < nmat && mats[t.matId].type == FLX_BXDF_DIFFUSE) areaDiffuse += a;
        }
        // Round 3 (persistent closest hit, RAW commit in the pass, shadow rays on the second stream; profiles/r03_fuse_set_ab.txt, same box, diffuse ->
        // all): courtyard (65 % diffuse) 2158 -> 2258 and 2221 -> 2274 Mrays/s at 1440p, 2088 -> 2167 and 2189 -> 2200 at 2160p -- a third of
        // its paths took the second trip -- kitchen (96 %) 5297 -> 5152 and 5485 -> 5198.  Hence all types below 3/4 diffuse (round 2: 1/2).
        c->fuseSet = (areaAll > 0.0 && areaDiffuse < 0.75 * areaAll) ? 31 : 1;
        // ... and whether the all-types pass sorts its material step by BSDF type inside each block (logic.hip: LOGIC_REGROUP, k_logic<31, true, true>).  Round 5's
        // build of it needed 119 VGPRs (4 waves per SIMD) and paid only where one type dominates (profiles/r05_regroup_ab.txt); as a template instance of its own,
        // compiled for 5 blocks per CU, it fits 96 VGPRs without scratch, and the same-box A/B at 16 M paths reads (profiles/r06_regroup_ab.txt, off -> on, Mrays/s):
        // conference 5392 -> 5678 and 5376 -> 5654 (+5.2 %), courtyard-1440p 2512 -> 2503 and 2483 -> 2491, egyptcat 6079 -> 6074 and 6009 -> 6042 (both +-0.5 %: the
        // box's spread).  On whenever the all-types pass runs; option "regroup" overrides.
        c->regroupAuto = 1;
        c->regroup = c->regroupOpt >= 0 ? c->regroupOpt : c->regroupAuto;
        // ... and the order in which the fused pass lists the continuing paths in the extension queue (logic.hip: k_queue_build): one
        // segment per material queue, as the separate kernels append them, or all of them by path id.  Same-box A/B, Mrays/s segments ->
        // path id: conference 4318 -> 4446 (+3 %: three BSDF types of similar weight, the segments cut the id order into thirds),
        // kitchen 4278 -> 4230, courtyard 1678 -> 1652 (one dominant type: its segment IS the id order, and the small segments of the
        // other types are rays leaving the same few objects).  Option "ext_order" overrides.
        // Round 4, 8 M paths (profiles/r04_ext_order_ab.txt, same box): with the diffuse-only pass the kitchen's closest-hit kernel takes 1.056 ms on
        // the per-queue segments, 1.037 by path id, 1.035 with the regenerated paths merged in (ext_order 2: the queue is the identity permutation in
        // the steady state; step +1 %); conference and courtyard (all-types pass) do not move between 1 and 2.  Hence 2 with the diffuse-only pass.
        c->extOrder = c->fuseSet == 31 ? 1 : 2;
    }

    // 1. leaf triangle records, in index-list order (a leaf is a contiguous run of the list)
    std::vector<TriRec> trirecs(nidx);
    for (size_t s = 0; s < nidx; s++) {
        NEED(c, indices[s] < ntris, "flx_upload_scene: index out of range");
        const flx_triangle &t = tris[indices[s]];
        int idx = (int)indices[s], zero = 0;
        float fi, fz; memcpy(&fi, &idx, 4); memcpy(&fz, &zero, 4);
        trirecs[s].a = make_float4(t.v0.p.x, t.v0.p.y, t.v0.p.z, fi);
        trirecs[s].b = make_float4(t.v1.p.x, t.v1.p.y, t.v1.p.z, fz);
        trirecs[s].c = make_float4(t.v2.p.x, t.v2.p.y, t.v2.p.z, 0.0f);
    }
    // 2. inner-node records: both child boxes + refs; DFS numbering of inner nodes only
    // Record numbering ("sibling pairs"): the vector L1 and the L2 move 128-B lines, a BNode is 64 B.  The two inner children
    // of a node get the two halves of ONE 128-B-aligned line, allocated when their parent is numbered (pre-order, so a
    // root-to-leaf path stays roughly contiguous): descending into the nearer child brings the farther child's record
    // along, and the later pop of that sibling finds its line in L1/L2 instead of missing.  Single inner children are
    // packed two to a line.  Option node_layout 0 (set before the upload) = plain DFS numbering, for A/B.
    std::vector<int32_t> innerId(nnodes, -1);
    uint32_t ninner = 0, nrecords = 0;
    for (size_t i = 0; i < nnodes; i++) if (nodes[i].nPrims == 0) ninner++;
    const int nodeLayout = c->nodeLayout;
    if (nodeLayout == 0 || ninner == 0) {
        for (size_t i = 0; i < nnodes; i++) if (nodes[i].nPrims == 0) innerId[i] = (int32_t)nrecords++;     // reference DFS order
    } else {
        std::vector<uint32_t> todo; todo.reserve(128);
        innerId[0] = 0; nrecords = 2;                                   // the root's line-mate stays empty
        int32_t spare = -1;                                             // free half of a line opened for a single inner child
        todo.push_back(0);
        while (!todo.empty()) {
            const uint32_t i = todo.back(); todo.pop_back();
            const uint32_t l = i + 1, r = nodes[i].iStartOrRight;
            NEED(c, l < nnodes && r < nnodes, "flx_upload_scene: child index out of range");
            const bool li = nodes[l].nPrims == 0, ri = nodes[r].nPrims == 0;
            // an inner child that already has a record is reachable twice: cyclic or shared node array (e.g. a corrupt cache file)
            NEED(c, !(li && innerId[l] >= 0) && !(ri && innerId[r] >= 0) && r > i, "flx_upload_scene: malformed node array (node reachable twice)");
            if (li && ri) { innerId[l] = (int32_t)nrecords; innerId[r] = (int32_t)nrecords + 1; nrecords += 2; }
            else if (li || ri) {
                const uint32_t ch = li ? l : r;
                if (spare >= 0) { innerId[ch] = spare; spare = -1; }
                else { innerId[ch] = (int32_t)nrecords; spare = (int32_t)nrecords + 1; nrecords += 2; }
            }
            if (ri) todo.push_back(r);                                  // left subtree first
            if (li) todo.push_back(l);
        }
        for (size_t i = 0; i < nnodes; i++) NEED(c, nodes[i].nPrims != 0 || innerId[i] >= 0, "flx_upload_scene: inner node unreachable from the root");
    }
    auto childRef = [&](uint32_t ni, bool &ok) -> uint32_t {
        if (ni >= nnodes) { ok = false; return 0; }
        const flx_node &n = nodes[ni];
        if (n.nPrims == 0) return (uint32_t)innerId[ni];
        if ((size_t)n.iStartOrRight + n.nPrims > nidx) { ok = false; return 0; }
        int cnt = n.nPrims; float fc; memcpy(&fc, &cnt, 4);
        trirecs[n.iStartOrRight].b.w = fc;               // leaf count lives in the run's first record
        { uint32_t one = 1u; float fl; memcpy(&fl, &one, 4); trirecs[n.iStartOrRight + n.nPrims - 1].c.w = fl; }   // end-of-run flag (trace_mode 3)
        return FLX_LEAF_BIT | n.iStartOrRight;
    };
    std::vector<BNode> bnodes(ninner ? nrecords : 1);
    memset(bnodes.data(), 0, bnodes.size() * sizeof(BNode));
    bool ok = true;
    if (ninner == 0) {
        // the whole scene is one leaf: synthetic root whose two children are that leaf
        BNode &b = bnodes[0];
        const flx_node &n = nodes[0];
        const float mn[3] = {n.bmin.x, n.bmin.y, n.bmin.z}, mx[3] = {n.bmax.x, n.bmax.y, n.bmax.z};
        for (int k = 0; k < 3; k++) { b.lmin[k] = b.rmin[k] = mn[k]; b.lmax[k] = b.rmax[k] = mx[k]; }
        b.left = b.right = childRef(0, ok); b.pad[0] = b.pad[1] = 0;
    } else {
        for (size_t i = 0; i < nnodes; i++) {
            if (nodes[i].nPrims != 0) continue;
            BNode &b = bnodes[innerId[i]];
            uint32_t l = (uint32_t)i + 1, r = nodes[i].iStartOrRight;
            NEED(c, l < nnodes && r < nnodes, "flx_upload_scene: child index out of range");
            const flx_node &ln = nodes[l], &rn = nodes[r];
            b.lmin[0] = ln.bmin.x; b.lmin[1] = ln.bmin.y; b.lmin[2] = ln.bmin.z; b.lmax[0] = ln.bmax.x; b.lmax[1] = ln.bmax.y; b.lmax[2] = ln.bmax.z;
            b.rmin[0] = rn.bmin.x; b.rmin[1] = rn.bmin.y; b.rmin[2] = rn.bmin.z; b.rmax[0] = rn.bmax.x; b.rmax[1] = rn.bmax.y; b.rmax[2] = rn.bmax.z;
            b.left = childRef(l, ok); b.right = childRef(r, ok); b.pad[0] = b.pad[1] = 0;
        }
    }
    NEED(c, ok, "flx_upload_scene: malformed node array");
    // 3. shading records per ORIGINAL triangle index
    std::vector<ShadeRec> shade(ntris);
    for (size_t i = 0; i < ntris; i++) {
        const int m = tris[i].matId;
        NEED(c, m >= 0 && (size_t)m < nmat, "flx_upload_scene: triangle material id out of range");
        float4 w[10]; memcpy(w, &tris[i], sizeof w);       // the wire triangle as the refit's shade pass reads it
        flxrf::rf_shade_rec(w, shade[i].a, shade[i].b, shade[i].c, shade[i].d);
    }
    // 4. the 4-wide quantised tree over the same leaves (flx_wide.h) + the depth of the binary tree (stack-spill sizing)
    // (Round 4 re-optimised the inner topology over the reference's leaves before this collapse -- subtree reinsertion, archived in
    //  scripts/experiments/flx_wide_opt.h: node visits -0.8 % kitchen / -5 % conference / -1.3 % courtyard on the device, both traversal
    //  kernels within 0-3 %, 25 s more upload time on the courtyard; below the bar, not shipped.  profiles/r04_wide_opt_ab.txt)
    flxw::WideTree wide;
    { const char *werr = nullptr; if (!flxw::build_wide(nodes, nnodes, tris, ntris, indices, nidx, wide, &werr)) { c->err = std::string("flx_upload_scene: ") + werr; return 1; } }
    uint32_t binDepth = 1;
    std::vector<uint16_t> depth(nnodes, 0);
    {   // nodes are in DFS order with parent < child (checked above for the right child; the left child is i + 1)
        for (size_t i = 0; i < nnodes; i++) {
            if (nodes[i].nPrims != 0) continue;
            const uint32_t l = (uint32_t)i + 1, r = nodes[i].iStartOrRight;
            NEED(c, r > i && r < nnodes && l < nnodes, "flx_upload_scene: malformed node array");
            const uint16_t dd = (uint16_t)(depth[i] + 1);
            NEED(c, dd < 4096, "flx_upload_scene: tree deeper than 4095 levels");
            depth[l] = dd; depth[r] = dd;
            if (dd > binDepth) binDepth = dd;
        }
    }
    uint32_t spillLevels = 1;
    if (binDepth + 1 > LDS_LEVELS) spillLevels = binDepth + 1 - LDS_LEVELS;
    // the 4-wide kernels page whole groups of 8 levels between their LDS ring and level-indexed spill rows (flx_trace4.h)
    if (wide.maxStack > WIDE_LDS_LEVELS - 4 && wide.maxStack + 8 > spillLevels) spillLevels = wide.maxStack + 8;

    // 5. what a bottom-up pass over the same topology needs (flx_update_triangles, refit.hip): the records of each depth of both trees, where
    // the wide leaf blocks and their triangles start.  (Level 0 of both lists holds the root ALONE, so the first listed record is the root:
    // flx_tree_cost's kernels take A_root from list entry 0, tree_cost.hip.)
    RefitTables rf;
    std::vector<uint32_t> blevel, wlevel, wtriOff;
    std::vector<float4> wexact;
    {
        auto byDepth = [](size_t n, auto depthOf, auto idOf, std::vector<uint32_t> &list, std::vector<uint32_t> &start) {
            uint32_t levels = 0;
            for (size_t i = 0; i < n; i++) if (idOf(i) >= 0 && depthOf(i) + 1 > levels) levels = depthOf(i) + 1;
            start.assign(levels + 1, 0);
            for (size_t i = 0; i < n; i++) if (idOf(i) >= 0) start[depthOf(i) + 1]++;
            for (uint32_t l = 0; l < levels; l++) start[l + 1] += start[l];
            list.resize(start[levels]);
            std::vector<uint32_t> fill(start.begin(), start.end() - 1);
            for (size_t i = 0; i < n; i++) if (idOf(i) >= 0) list[fill[depthOf(i)]++] = (uint32_t)idOf(i);
        };
        if (ninner == 0) { blevel.assign(1, 0); rf.blevelStart = {0, 1}; }            // the synthetic root
        else byDepth(nnodes, [&](size_t i) { return (uint32_t)depth[i]; }, [&](size_t i) { return (int64_t)innerId[i]; }, blevel, rf.blevelStart);
        if (!(wide.rootRef & FLX_WIDE_LEAF_BIT))
            byDepth(wide.nodes.size(), [&](size_t i) { return wide.nodeDepth[i]; }, [&](size_t i) { return (int64_t)i; }, wlevel, rf.wlevelStart);
        // the exact box of a wide node is its binary node's: what the parent's grid was quantised from.  A full refit rewrites all of them, a
        // subset refit reads those of the children it does not touch (refit.hip)
        wexact.resize(2 * wide.nodes.size());
        for (size_t i = 0; i < wide.nodes.size(); i++) {
            const flx_node &b = nodes[wide.nodeBin[i]];
            wexact[2 * i] = make_float4(b.bmin.x, b.bmin.y, b.bmin.z, 0.0f); wexact[2 * i + 1] = make_float4(b.bmax.x, b.bmax.y, b.bmax.z, 0.0f);
        }
        for (uint32_t off : wide.leafOffset) {
            int cnt; memcpy(&cnt, &wide.leafdata[off].w, 4);
            for (int k = 0; k < cnt; k++) wtriOff.push_back(off + 2 + 3 * (uint32_t)k);
        }
        NEED(c, ntris < 0xFFFFFFFFull && nidx + wtriOff.size() < 0xFFFFFFFFull, "flx_upload_scene: more than 2^32 triangle records");
        rf.ntris = (uint32_t)ntris; rf.nidx = (uint32_t)nidx; rf.nmat = (uint32_t)nmat; rf.nwtri = (uint32_t)wtriOff.size(); rf.nwleaf = (uint32_t)wide.leafOffset.size();
    }

    // Allocate and fill the new scene first; the previous one is released (and c->sc switched) only when everything succeeded,
    // so a failed upload leaves the context on its old scene instead of on dangling pointers.
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
    std::vector<void *> fresh, freshSpill;
    auto bail = [&]() { freeAll(fresh); freeAll(freshSpill); return 1; };
    BNode *dB; TriRec *dT; ShadeRec *dS; flx_triangle *dTri; flx_material *dM; flx_texdesc *dD; uint8_t *dX; flxw::WNode *dW; float4 *dL;
    if (dalloc(c, fresh, &dB, bnodes.size()) || dalloc(c, fresh, &dT, trirecs.size() + 1) || dalloc(c, fresh, &dS, shade.size()) ||
        dalloc(c, fresh, &dTri, ntris) || dalloc(c, fresh, &dM, nmat) || dalloc(c, fresh, &dD, ntex) || dalloc(c, fresh, &dX, texbytes + 4) ||
        dalloc(c, fresh, &dW, wide.nodes.size()) || dalloc(c, fresh, &dL, wide.leafdata.size() + 4) ||
        dalloc(c, fresh, &rf.blevel, blevel.size()) || dalloc(c, fresh, &rf.wlevel, wlevel.size()) || dalloc(c, fresh, &rf.wtriOff, wtriOff.size()) ||
        dalloc(c, fresh, &rf.wleafOff, wide.leafOffset.size()) || dalloc(c, fresh, &rf.wexact, 2 * wide.nodes.size()) || dalloc(c, fresh, &rf.valid, 4))
        return bail();
    uint32_t *sp1 = c->spill, *sp2 = c->spill2;
    const size_t lanes = ((size_t)c->numTasks + 255) / 256 * 256 + 1024;
    const bool newSpill = spillLevels > c->spillLevels || !c->spill;
    if (newSpill && (dalloc(c, freshSpill, &sp1, lanes * spillLevels) || dalloc(c, freshSpill, &sp2, lanes * spillLevels))) return bail();
    UPCHK(hipMemcpy(dB, bnodes.data(), bnodes.size() * sizeof(BNode), hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(dT, trirecs.data(), trirecs.size() * sizeof(TriRec), hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(dS, shade.data(), shade.size() * sizeof(ShadeRec), hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(dTri, tris, ntris * sizeof(flx_triangle), hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(dM, materials, nmat * sizeof(flx_material), hipMemcpyHostToDevice));
    if (ntex) UPCHK(hipMemcpy(dD, texdesc, ntex * sizeof(flx_texdesc), hipMemcpyHostToDevice));
    if (texbytes) UPCHK(hipMemcpy(dX, texdata, texbytes, hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(dW, wide.nodes.data(), wide.nodes.size() * sizeof(flxw::WNode), hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(dL, wide.leafdata.data(), wide.leafdata.size() * sizeof(float4), hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(rf.blevel, blevel.data(), blevel.size() * 4, hipMemcpyHostToDevice));
    if (!wlevel.empty()) UPCHK(hipMemcpy(rf.wlevel, wlevel.data(), wlevel.size() * 4, hipMemcpyHostToDevice));
    if (!wtriOff.empty()) UPCHK(hipMemcpy(rf.wtriOff, wtriOff.data(), wtriOff.size() * 4, hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(rf.wexact, wexact.data(), wexact.size() * sizeof(float4), hipMemcpyHostToDevice));
    if (rf.nwleaf) UPCHK(hipMemcpy(rf.wleafOff, wide.leafOffset.data(), (size_t)rf.nwleaf * 4, hipMemcpyHostToDevice));
    freeAll(c->sceneAllocs);
    c->sceneAllocs.swap(fresh);
    c->rf = std::move(rf);
    c->ob.release();                                      // objects are defined over the triangles of one upload (flx_objects_define)
    {   // the emissive triangles, ascending (flx_mesh_light.h): the list depends on the materials, which only this call brings
        const flx_material *mats = (const flx_material *)materials;
        c->ml.releaseBuffers();
        c->ml.list.clear();
        for (size_t i = 0; i < ntris; i++) { const flx_vec3 &ke = mats[tris[i].matId].Ke; if (flxml::ml_is_emissive(ke.x, ke.y, ke.z)) c->ml.list.push_back((uint32_t)i); }
        c->ml.state.sceneUploaded((uint32_t)c->ml.list.size());
    }
    c->temporal.state.definitionChanged(c->motionHistory);
    c->temporal.state.sceneUploaded(c->deformHistory != 0);
    if (newSpill) { freeAll(c->spillAllocs); c->spillAllocs.swap(freshSpill); c->spill = sp1; c->spill2 = sp2; c->spillLevels = spillLevels; }
    c->sc.bnodes = dB; c->sc.trirecs = dT; c->sc.shade = dS; c->sc.tris = dTri; c->sc.materials = dM; c->sc.texdesc = dD; c->sc.texdata = dX;
    c->sc.rootRef = 0;
    c->sc.wnodes = dW; c->sc.wleaf = dL; c->sc.wrootRef = wide.rootRef;
    {   // flx_trace4.h, WRay::setup: which clamp of 1 / dir keeps (o - orig) * dinv finite for this scene
        const flx_node &r0 = nodes[0];
        const float ext[6] = {r0.bmin.x, r0.bmin.y, r0.bmin.z, r0.bmax.x, r0.bmax.y, r0.bmax.z};
        float m = 0.0f; for (float v : ext) m = std::fabs(v) > m ? std::fabs(v) : m;
        c->sc.wideClamp = wideClampFor(m);
    }
    // the exactness argument of the wide any-hit traversal needs nested boxes (flx_wide.h); a tree without them (no builder of
    // ours or of the reference produces one) is traversed with the binary kernels
    c->wideOK = wide.nested;
    c->wideInfo[0] = (uint32_t)wide.nodes.size(); c->wideInfo[1] = (uint32_t)(wide.leafdata.size()); c->wideInfo[2] = wide.maxStack; c->wideInfo[3] = wide.nested ? 1u : 0u;
    c->wideInfo[4] = binDepth; c->wideInfo[5] = spillLevels; c->wideInfo[6] = (uint32_t)bnodes.size(); c->wideInfo[7] = wide.maxLeafCount;
    pickSchedule(c);
    if (splitPrepare(c)) return 1;                        // (wideOK is known now: the records of the split any-hit launch, api.hip)
    return meshLightsSync(c);                            // option "mesh_lights": the table of the new scene, on the stream
}

int flx_upload_envmap(flx_ctx *c, const float *rgb, int w, int h, const float *prob, const int *alias, const float *pdf)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, rgb && prob && alias && pdf && w > 0 && h > 0, "flx_upload_envmap: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    std::vector<float4> rgba(n);
    for (size_t i = 0; i < n; i++) rgba[i] = make_float4(rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2], 1.0f);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the probability and alias tables of the reference (src/envmap.cpp:31-114) merged into one record per texel (flx_device.h: aliasRec); the pdf table
    // stays as it is (env_map_pdf, and the per-texel NEE table below is built from it).  An alias outside the table (a malformed upload) is clamped like the kernel's own index clamp.
    std::vector<float2> rec(n);
    for (size_t i = 0; i < n; i++) {
        int a = alias[i]; if (a < 0) a = 0; if ((size_t)a >= n) a = (int)n - 1;
        float af; memcpy(&af, &a, 4);
        rec[i] = make_float2(prob[i], af);
    }
    // The new map is allocated and filled first; the previous one is released and c->sc switched only when every allocation, copy and the table
    // kernel have succeeded, so a failed upload leaves the context on its old map instead of on dangling pointers (round 5's advisor).
    std::vector<void *> fresh;
    float4 *dR; float2 *dRec; float *dF; float4 *dNee;
    auto bail = [&]() { freeAll(fresh); return 1; };
    if (dalloc(c, fresh, &dR, n) || dalloc(c, fresh, &dRec, n) || dalloc(c, fresh, &dF, n) || dalloc(c, fresh, &dNee, 2 * n)) return bail();
    UPCHK(hipMemcpy(dR, rgba.data(), n * 16, hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(dRec, rec.data(), n * 8, hipMemcpyHostToDevice));
    UPCHK(hipMemcpy(dF, pdf, n * 4, hipMemcpyHostToDevice));
    Scene tmp = c->sc;
    tmp.envRGBA = dR; tmp.aliasRec = dRec; tmp.pdfTable = dF; tmp.envW = w; tmp.envH = h;
    launch_env_nee_table(c->stream, tmp, dNee, (uint32_t)n); UPCHK(hipGetLastError());
    UPCHK(hipStreamSynchronize(c->stream));
    freeAll(c->envAllocs);
    c->envAllocs.swap(fresh);
    c->sc.envRGBA = dR; c->sc.aliasRec = dRec; c->sc.pdfTable = dF; c->sc.envW = w; c->sc.envH = h; c->sc.neeRec = dNee;
    return 0;
}

} // extern "C"
