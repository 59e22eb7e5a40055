// feature_state_cpu.cpp -- tests/feature_state_cases.py through csrc/flx_feature_state.h without a GPU: each event does to the state types what
// the entry point of that name does to them in csrc/api*.hip (the same checks in the same order, the same transition), everything else of the
// context reduced to what those lines read: the options, whether objects are defined, the image size.  Reads the script of
// feature_state_cases.script() on stdin; prints per case
//     NAME T0 T1 O0 O1 H L Hm D moved known knownCap          (known / knownCap: one digit per object, "-" without objects)
// Exit status 2: an event the script calls accepted was refused or the other way round, or a slot held an object plane without a G-buffer.
#include "../fluctus_amd/csrc/flx_feature_state.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace flxd;

struct Model {
    TemporalState temporal; PoseState pose; ActiveListState ad;
    bool dnHave = false;                        // flx_ctx::Denoise::have, which stays with its buffers: set by flx_denoise, released with the framebuffers
    bool motionHistory = false, moments = false, denoiser = false, objects = false;
    uint32_t W = 0, H = 0, pixels = 0;
    flx_camera cam = {};

    void releaseFrameFeatures() { dnHave = false; temporal = TemporalState(); ad = ActiveListState(); }
    void setParams(uint32_t w, uint32_t h)
    {
        if (w != W || h != H) ad.dropped();
        W = w; H = h;
        if (w * h != pixels) { releaseFrameFeatures(); pixels = w * h; }       // allocFrame
    }
    void updateTriangles(bool byPose)
    {
        ad.dropped();
        temporal.trianglesMoved(byPose, motionHistory);
        if (!byPose) pose.trianglesSetDirectly();
    }
    // true: the call is accepted
    bool event(std::istringstream &in)
    {
        std::string k; in >> k;
        if (k == "opt") {
            std::string name; int v = 0; in >> name >> v;
            if (name == "motion_history") { if (!v) temporal.motionHistoryOff(); motionHistory = v; }
            else if (name == "moments") { if (!v) ad.dropped(); moments = v; }
            else if (name == "denoiser") denoiser = v;
            else return false;
        } else if (k == "define") {
            uint32_t n = 0; in >> n;
            pose = PoseState(); pose.defined(n); objects = n != 0;
            temporal.definitionChanged(motionHistory);
        } else if (k == "pose") {
            if (!objects) return false;
            std::vector<uint32_t> ids; std::vector<float> x;
            for (std::string tok; in >> tok;) {
                const float t = tok.back() == 'T' ? 0.1f : 0.0f, m[12] = {1, 0, 0, t, 0, 1, 0, 0, 0, 0, 1, 0};
                ids.push_back((uint32_t)std::stoul(tok)); x.insert(x.end(), m, m + 12);
            }
            updateTriangles(true);
            pose.posed(ids.data(), x.data(), (uint32_t)ids.size());
        } else if (k == "update" || k == "subset") updateTriangles(false);
        else if (k == "gbuffer") temporal.traced(cam, W, H, motionHistory && objects);
        else if (k == "gb_write") { int s = 0; in >> s; temporal.written(s, cam, W, H, motionHistory); }
        else if (k == "obj_write") {
            int s = 0; in >> s;
            if (!motionHistory || !temporal.holdsSized(s, W, H)) return false;
            temporal.objectsWritten(s);
        } else if (k == "capture") {
            if (!temporal.holds(0) || !temporal.holdsSized(0, W, H)) return false;
            temporal.captured(moments);
            pose.captured();
        } else if (k == "upload" || k == "upload_refused") {
            ad.dropped();
            if (k == "upload_refused") return false;
            pose = PoseState(); objects = false;
            temporal.definitionChanged(motionHistory);
        } else if (k == "resize") { uint32_t w = 0, h = 0; in >> w >> h; setParams(w, h); }
        else if (k == "partition" || k == "mk_reset" || k == "adaptive_clear") ad.dropped();
        else if (k == "adaptive_update") { if (!moments) return false; ad.pix = pixels; ad.installed(pixels); }
        else if (k == "active_write") { uint32_t n = 0; in >> n; ad.pix = pixels; ad.installed(n); }
        else if (k == "denoise") { if (!denoiser) return false; dnHave = true; }
        else { fprintf(stderr, "unknown event %s\n", k.c_str()); exit(2); }
        return true;
    }
    // what flx_reproject's table comes to (flx_reproject_motion.h: rm_make_table returns it): an object posed now whose pose at the capture is unknown or other bytes
    bool moved() const
    {
        const PoseState::Poses p = pose.sinceCapture();
        for (size_t o = 0; o < pose.count(); o++)
            if (p.nowKnown[o] && (!p.atCaptureKnown[o] || memcmp(p.atCapture + 12 * o, p.now + 12 * o, 48) != 0)) return true;
        return false;
    }
};

int main()
{
    Model m; std::string name, line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (line.rfind("case ", 0) == 0) {
            std::string k; uint32_t w = 0, h = 0; in >> k >> name >> w >> h;
            m = Model(); m.setParams(w, h);
        } else if (line == "end") {
            const TemporalState &t = m.temporal;
            const PoseState::Poses p = m.pose.sinceCapture();
            std::string known = "-", knownCap = "-";
            if (m.pose.count()) { known.clear(); knownCap.clear(); }
            for (size_t o = 0; o < m.pose.count(); o++) { known += char('0' + p.nowKnown[o]); knownCap += char('0' + p.atCaptureKnown[o]); }
            printf("%s %d %d %d %d %d %d %d %d %d %s %s\n", name.c_str(), t.holds(0), t.holds(1), t.holdsObjects(0), t.holdsObjects(1), t.hist, m.ad.have,
                   t.histMom, m.dnHave, m.objects && m.moved(), known.c_str(), knownCap.c_str());
        } else {
            const bool refused = line.rfind("refused ", 0) == 0;
            if (refused) { std::string k; in >> k; }
            if (m.event(in) == refused) { fprintf(stderr, "%s: `%s` was %s\n", name.c_str(), line.c_str(), refused ? "accepted" : "refused"); return 2; }
            for (int s = 0; s < 2; s++)
                if (m.temporal.slot[s].objects && !m.temporal.slot[s].traced) { fprintf(stderr, "%s: slot %d has an object plane without a G-buffer after `%s`\n", name.c_str(), s, line.c_str()); return 2; }
        }
    }
    return 0;
}
