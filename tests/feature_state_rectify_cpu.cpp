// feature_state_rectify_cpu.cpp -- tests/feature_state_rectify_cases.py through csrc/flx_feature_state.h without a GPU, as
// tests/feature_state_cpu.cpp runs its table: each event does to TemporalState what the entry point of that name does to it in csrc/api*.hip (the
// same checks in the same order, the same transition), everything else of the context reduced to what those lines read.  Reads the script of
// feature_state_rectify_cases.script() on stdin; prints per case
//     NAME T0 Mk MkMom Live
// Exit status 2: an event the script calls accepted was refused or the other way round, or a mark had moments without being a mark.
#include "../fluctus_amd/csrc/flx_feature_state.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace flxd;

struct Model {
    TemporalState temporal;
    bool motionHistory = false, moments = false, objects = false;
    uint32_t W = 0, H = 0, pixels = 0;
    flx_camera cam = {};

    void setParams(uint32_t w, uint32_t h)
    {
        if (w != W || h != H) temporal.imageResized();
        W = w; H = h;
        if (w * h != pixels) { temporal = TemporalState(); pixels = w * h; }       // allocFrame: releaseFrameFeatures
    }
    // true: the call is accepted
    bool event(std::istringstream &in)
    {
        std::string k; in >> k;
        if (k == "opt") {
            std::string name; int v = 0; in >> name >> v;
            if (name == "motion_history") { if (!v) temporal.motionHistoryOff(); motionHistory = v; }
            else if (name == "moments") moments = v;
            else return false;
        } else if (k == "define") {
            uint32_t n = 0; in >> n;
            objects = n != 0;
            temporal.definitionChanged(motionHistory);
        } else if (k == "pose") { if (!objects) return false; temporal.trianglesMoved(true, motionHistory, false); }
        else if (k == "update" || k == "subset") temporal.trianglesMoved(false, motionHistory, false);
        else if (k == "gbuffer") { temporal.traced(cam, W, H, motionHistory && objects); temporal.baryWith(0, false); }
        else if (k == "gb_write") { int s = 0; in >> s; temporal.written(s, cam, W, H, motionHistory); temporal.baryWith(s, false); }
        else if (k == "capture") {
            if (!temporal.holds(0) || !temporal.holdsSized(0, W, H)) return false;
            temporal.captured(moments);
        } else if (k == "upload") { objects = false; temporal.definitionChanged(motionHistory); temporal.sceneUploaded(false); }
        else if (k == "resize") { uint32_t w = 0, h = 0; in >> w >> h; setParams(w, h); }
        else if (k == "partition") temporal.partitionSet();
        else if (k == "mk_reset" || k == "wf_reset") temporal.accumulationReset();
        else if (k == "mark") {
            if (!temporal.holdsSized(0, W, H)) return false;
            temporal.marked(moments);
        } else if (k == "rectify" || k == "rectify_bad") {
            if (k == "rectify_bad") return false;                                   // the parameters are checked first
            if (!temporal.hasMark() || !temporal.markLive() || !temporal.holdsSized(0, W, H)) return false;
        } else if (k == "write_pixels") { }
        else { fprintf(stderr, "unknown event %s\n", k.c_str()); exit(2); }
        return true;
    }
    bool rectifyWouldRun() const { return temporal.hasMark() && temporal.markLive() && temporal.holdsSized(0, W, H); }
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
            printf("%s %d %d %d %d\n", name.c_str(), t.holds(0), t.hasMark(), t.markHasMoments(), m.rectifyWouldRun());
        } else {
            const bool refused = line.rfind("refused ", 0) == 0;
            if (refused) { std::string k; in >> k; }
            const TemporalState before = m.temporal;
            if (m.event(in) == refused) { fprintf(stderr, "%s: `%s` was %s\n", name.c_str(), line.c_str(), refused ? "accepted" : "refused"); return 2; }
            if (refused && (before.mark != m.temporal.mark || before.markMom != m.temporal.markMom || before.hist != m.temporal.hist ||
                            before.slot[0].traced != m.temporal.slot[0].traced)) { fprintf(stderr, "%s: the refused `%s` changed the state\n", name.c_str(), line.c_str()); return 2; }
            if (m.temporal.markMom && !m.temporal.mark) { fprintf(stderr, "%s: moments of no mark after `%s`\n", name.c_str(), line.c_str()); return 2; }
        }
    }
    return 0;
}
