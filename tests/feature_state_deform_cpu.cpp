// feature_state_deform_cpu.cpp -- tests/feature_state_deform_cases.py through csrc/flx_feature_state.h without a GPU, in the way
// feature_state_cpu.cpp runs its table: each event does to TemporalState what the entry point of that name does to it in csrc/api*.hip under
// option "deform_history" (the same checks in the same order, the same transition), everything else of the context reduced to what those lines
// read: the two options, whether objects are defined, the image size.  Reads the script of feature_state_deform_cases.script() on stdin; prints
// per case
//     NAME T0 T1 B0 B1 H S snapshots
// Exit status 2: an event the script calls accepted was refused or the other way round, or a flag stood without what it needs (a plane without
// a G-buffer, a snapshot without a history).
#include "../fluctus_amd/csrc/flx_feature_state.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace flxd;

struct Model {
    TemporalState temporal;
    bool motionHistory = false, deformHistory = false, objects = false;
    uint32_t W = 0, H = 0, pixels = 0;
    int snapshots = 0;                          // launches of k_snapshot_positions
    flx_camera cam = {};

    void setParams(uint32_t w, uint32_t h)
    {
        W = w; H = h;
        if (w * h != pixels) { temporal = TemporalState(); pixels = w * h; }       // allocFrame: releaseFrameFeatures
    }
    void updateTriangles(bool byPose)           // api_refit.hip, behind the validation
    {
        if (temporal.needsSnapshot(deformHistory)) snapshots++;
        temporal.trianglesMoved(byPose, motionHistory, deformHistory);
    }
    // true: the call is accepted
    bool event(std::istringstream &in)
    {
        std::string k; in >> k;
        if (k == "opt") {
            std::string name; int v = 0; in >> name >> v;
            if (name == "motion_history") { if (v && deformHistory) return false; if (!v) temporal.motionHistoryOff(); motionHistory = v; }
            else if (name == "deform_history") { if (v && motionHistory) return false; if (!v) temporal.deformHistoryOff(); deformHistory = v; }
            else return false;
        } else if (k == "define") { uint32_t n = 0; in >> n; objects = n != 0; temporal.definitionChanged(motionHistory); }
        else if (k == "pose") { if (!objects) return false; updateTriangles(true); }
        else if (k == "update" || k == "subset") updateTriangles(false);
        else if (k == "update_nan") return false;                                   // refused by the validation: nothing above has run
        else if (k == "gbuffer") { temporal.traced(cam, W, H, motionHistory && objects); temporal.baryWith(0, deformHistory); }
        else if (k == "gb_write") { int s = 0; in >> s; temporal.written(s, cam, W, H, motionHistory); temporal.baryWith(s, deformHistory); }
        else if (k == "bary_write") {
            int s = 0; in >> s;
            if (!deformHistory || !temporal.holdsSized(s, W, H)) return false;
            temporal.baryWritten(s);
        } else if (k == "capture") {
            if (!temporal.holds(0) || !temporal.holdsSized(0, W, H)) return false;
            temporal.captured(false);
        } else if (k == "reproject") {
            if (!temporal.hasHistory() || !temporal.holds(0) || !temporal.historyFits(W, H)) return false;
            if (temporal.followsMoves() && !(deformHistory && temporal.followsMovesReady())) return false;
        } else if (k == "upload") { objects = false; temporal.definitionChanged(motionHistory); temporal.sceneUploaded(deformHistory); }
        else if (k == "resize") { uint32_t w = 0, h = 0; in >> w >> h; setParams(w, h); }
        else { fprintf(stderr, "unknown event %s\n", k.c_str()); exit(2); }
        return true;
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
            printf("%s %d %d %d %d %d %d %d\n", name.c_str(), t.holds(0), t.holds(1), t.holdsBary(0), t.holdsBary(1), t.hasHistory(), t.followsMoves(), m.snapshots);
        } else {
            const bool refused = line.rfind("refused ", 0) == 0;
            if (refused) { std::string k; in >> k; }
            const TemporalState before = m.temporal;
            if (m.event(in) == refused) { fprintf(stderr, "%s: `%s` was %s\n", name.c_str(), line.c_str(), refused ? "accepted" : "refused"); return 2; }
            const TemporalState &t = m.temporal;
            auto same = [](const TemporalState::Slot &a, const TemporalState::Slot &b) { return a.traced == b.traced && a.objects == b.objects && a.bary == b.bary; };
            if (refused && (!same(before.slot[0], t.slot[0]) || !same(before.slot[1], t.slot[1]) || before.hist != t.hist || before.snap != t.snap)) { fprintf(stderr, "%s: the refused `%s` changed the state\n", name.c_str(), line.c_str()); return 2; }
            for (int s = 0; s < 2; s++)
                if ((t.slot[s].bary || t.slot[s].objects) && !t.slot[s].traced) { fprintf(stderr, "%s: slot %d has a plane without a G-buffer after `%s`\n", name.c_str(), s, line.c_str()); return 2; }
            if (t.snap && !t.hasHistory()) { fprintf(stderr, "%s: a snapshot without a history after `%s`\n", name.c_str(), line.c_str()); return 2; }
        }
    }
    return 0;
}
