// tracer_history_cpu.cpp -- tests/tracer_history_cases.py through host/history_state.hpp without a GPU: each event does to the HistoryState what
// the public Tracer call of that name does to it in host/tracer.cpp (the same transitions in the same order), everything else of the Tracer
// reduced to what those lines read and write: the parameters, the integrator in use, `iteration` and `paramsUpdatePending`; a device call
// becomes a letter.  Reads the script of tracer_history_cases.script() on stdin; prints per case
//     NAME TOKEN ... | have captured mark framesSinceGbuffer temporalFrames iteration pending switches delay history
// with one token per `frame` and per `move`:
//     frame   the device calls in order -- c flx_history_capture, g flx_gbuffer, r flx_reproject, m flx_history_mark, R flx_history_rectify; "."
//             none; "mk" the microkernel branch -- then @ and the frame the denoiser's schedule counts
//     move    mv: then k the history is kept, c the call captured it; "." neither
// switches: four digits temporal, motion, deform, rectify; delay: getRectifyDelay(); history: historyExists(params, integrator, posed = false).
// Exit status 2: an event the program does not know.
#include "../fluctus_amd/host/history_state.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using fluctus::HistoryState;

struct Model {
    HistoryState h;
    flx_render_params params;
    bool useWavefront = true, pending = true;
    uint32_t iteration = 0;
    std::string out;

    Model()
    {
        std::memset(&params, 0, sizeof(params));
        params.width = 32; params.height = 24; params.maxBounces = 4; params.worldRadius = 5.0f; params.useAreaLight = 1;
    }
    void geometryChanged() { params.worldRadius *= 1.01f; pending = true; h.dropped(); iteration = 0; }     // (worldRadius: re-derived from the moved tree)
    void toggle() { useWavefront = !useWavefront; iteration = 0; h.dropped(); }
    // Tracer::moveTriangles.  how: "" accepted, "refused" the device throws, "reupload" a blocking rebuild inside afterMove uploads a topology
    void move(bool switchOn, const std::string &how)
    {
        const HistoryState::MovePlan plan = h.beforeMove(switchOn, params, useWavefront);
        out += std::string(" mv:") + (plan.keep ? "k" : "") + (plan.captureNow ? "c" : "") + (plan.keep ? "" : ".");
        if (how == "refused") { if (plan.captureNow) pending = true; return; }
        geometryChanged();
        if (how == "reupload") geometryChanged();
        h.afterMove(plan.keep, how == "reupload");
    }
    void frame()
    {
        std::string t;
        bool reprojectNow = false;
        if (pending) {
            const HistoryState::ParamsPlan plan = h.paramsReachDevice(params, useWavefront);
            if (plan.captureNow) t += "c";
            pending = false; iteration = 0;
            if (plan.traceGbuffer) t += "g";
            reprojectNow = plan.reprojectNow;
        }
        const bool markNow = h.frameStarts(iteration, reprojectNow, useWavefront);
        if (!useWavefront) { out += " " + t + "mk@" + std::to_string(iteration); iteration++; return; }
        if (iteration == 0 && reprojectNow) t += "r";
        if (markNow) { t += "m"; h.marked(); }
        else if (h.rectifyDue(params.maxBounces)) { t += "R"; h.rectified(); }
        out += " " + (t.empty() ? std::string(".") : t) + "@" + std::to_string(h.denoiserSchedule(iteration));
        iteration++; h.frameRendered();
    }
    void event(std::istringstream &in)
    {
        std::string k; in >> k;
        if (k == "frame") { int n = 1; in >> n; for (int i = 0; i < n; i++) frame(); }
        else if (k == "temporal") {
            int on = 0; in >> on;
            h.temporalSet(on);
            if (!on && h.motion()) h.motionSet(false);
            if (!on && h.deform()) h.deformSet(false);
            if (!on && h.rectify()) h.rectifySet(false);
        }
        else if (k == "motion") { int on = 0; in >> on; h.motionSet(on); }
        else if (k == "deform") { int on = 0; in >> on; h.deformSet(on); }
        else if (k == "rectify") { int on = 0; in >> on; h.rectifySet(on); }
        else if (k == "delay") { uint32_t n = 0; in >> n; h.rectifyDelaySet(n); }
        else if (k == "params") {                            // getParams() + paramsChanged()
            std::string what; in >> what;
            if (what == "camera") params.camera.pos.x += 0.1f;
            else if (what == "light") params.areaLight.pos.x += 0.1f;
            else if (what == "bounces") in >> params.maxBounces;
            else if (what == "size") in >> params.width >> params.height;
            else if (what == "exposure") params.exposure += 0.5f;
            else { fprintf(stderr, "unknown parameter %s\n", what.c_str()); exit(2); }
            pending = true;
        }
        else if (k == "update_geometry") { std::string how; in >> how; move(h.deform(), how); }
        else if (k == "pose") { std::string how; in >> how; move(h.motion() || h.deform(), how); }
        else if (k == "adopt_rebuild") geometryChanged();    // adoptFinishedRebuild at the head of a move or of update()
        else if (k == "define") h.objectsDefined();
        else if (k == "envmap") { params.useEnvMap = 1; pending = true; h.dropped(); }
        else if (k == "toggle") toggle();
        else if (k == "mesh_lights" || k == "mesh_lights_wavefront") { iteration = 0; h.dropped(); }
        else if (k == "render_single" || k == "render_adaptive") {
            uint32_t spp = 0; in >> spp;
            if (useWavefront) toggle();
            params.useRoulette = 0;
            pending = false; h.dropped(); iteration += spp;
        }
        else if (k == "benchmark") { uint32_t n = 0; in >> n; iteration = 0; pending = false; h.dropped(); iteration += n; }
        else if (k == "init") { pending = true; iteration = 0; h.dropped(); }
        else if (k == "dropped") { pending = true; iteration = 0; h.dropped(); }      // what init() is measured against
        else if (k == "restart") iteration = 0;              // setDenoiser, setDenoiserMode: the accumulation restarts, the history is not told
        else { fprintf(stderr, "unknown event %s\n", k.c_str()); exit(2); }
    }
};

int main()
{
    Model m; std::string name, line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (line.rfind("case ", 0) == 0) { std::string k; in >> k >> name; m = Model(); }
        else if (line == "end") {
            const HistoryState &h = m.h;
            printf("%s%s | %d %d %d %u %u %u %d %d%d%d%d %u %d\n", name.c_str(), m.out.c_str(), h.haveGbuffer, h.capturedThisFrame, h.markPending,
                   h.framesSinceGbuffer, h.temporalFrames, m.iteration, m.pending, h.temporal(), h.motion(), h.deform(), h.rectify(),
                   h.rectifyDelayFrames(m.params.maxBounces), h.historyExists(m.params, m.useWavefront, false));
        } else m.event(in);
    }
    return 0;
}
