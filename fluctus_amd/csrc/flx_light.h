// flx_light.h -- the light sampling and MIS arithmetic of BOTH integrators (microkernel.hip, logic.hip), each formula once: an MIS estimator is
// unbiased only while the pdf its sampling branch divides by and the pdf its implicit-hit branch weighs with are the same function, so each pair
// shares one here -- the quad's area pdf quad_pdf_area, the lamps' (option "mesh_lights", flx_mesh_light.h) lamp_pdf_area, each turned into a
// solid-angle pdf by the one pdf_a_to_w -- and both integrators call it from both sides.  Where the integrators differ on
// purpose the difference is an argument, visible at the call site.
// Device only, like flx_shading.h; fp32 in the written order (no contraction).  The checkers (oracle/, tests/) restate all of this on their own.
#pragma once
#include "flx_bsdf.h"
#include "flx_launch.h"          // MeshLights, ml_vertices
#include "flx_mesh_light.h"

namespace flxd {

// ---- the two MIS weights (balance heuristic).  `pick` = the probability of choosing the light (kind), 1 in the microkernel.
__device__ __forceinline__ float mis_implicit(float lastPdfW, float directPdfW, float pick) { return lastPdfW / (lastPdfW + directPdfW * pick); }
__device__ __forceinline__ float mis_nee(float directPdfW, float pick, float bsdfPdfW) { return (directPdfW * pick) / (directPdfW * pick + bsdfPdfW); }
// the reference's weight of an implicit ENVIRONMENT hit (src/wf_logic.cl:84-107, src/mk_next_vertex.cl:72-93): the pick probability on the BSDF's
// side.  The complement of mis_nee only for pick = 1; kept as the reference has it wherever the reference's kinds are the only ones.
__device__ __forceinline__ float mis_implicit_env_reference(float lastPdfW, float pick, float directPdfW) { return (lastPdfW * pick) / (lastPdfW * pick + directPdfW); }

// ---- the tail of next event estimation: what one unoccluded light sample adds to the path's radiance
__device__ __forceinline__ f3 nee_contribution(f3 bsdf, f3 T, f3 Li, float cosTh, float directPdfW, float pick, float bsdfPdfW, bool mis)
{
    float weight = 1.0f;
    if (mis) weight = mis_nee(directPdfW, pick, bsdfPdfW);
    return bsdf * T * Li * weight * cosTh / (pick * directPdfW);
}
// ... with the BSDF evaluated here, toward the light (the microkernel; the wavefront's material step leaves bsdf and bsdfPdfW in the path state)
__device__ __forceinline__ f3 nee_eval(const Scene &sc, const SurfHit &h, const Mat &m, bool backface, f3 dirIn, f3 L, f3 T, f3 Li, float directPdfW, float pick, bool mis)
{
    const f3 brdf = bxdf_eval(sc, h, m, backface, dirIn, L);
    const float cosTh = fmaxf_(0.0f, dot(L, h.N));
    const float bsdfPdfW = fmaxf_(0.0f, bxdf_pdf(sc, h, m, backface, dirIn, L));
    return nee_contribution(brdf, T, Li, cosTh, directPdfW, pick, bsdfPdfW, mis);
}

// a light sample seen from `orig`: unit direction, the shadow ray's length, the cosine at the light (0: it faces away), and its solid-angle pdf
// from the area pdf and the distance that enters it -- evaluated where it is consumed (the microkernel traces the shadow ray first)
struct LightSample {
    f3 L; float rayLen, cosLight, pdfA, pdfDist;
    __device__ float pdfW() const { return pdf_a_to_w(pdfA, pdfDist, cosLight); }
};

// ---- the parametric quad (reference: sampleAreaLight)
__device__ __forceinline__ float quad_pdf_area(const flx_arealight &l) { return 1.0f / (4.0f * l.size.x * l.size.y); }
__device__ __forceinline__ float quad_pdf_w(const flx_arealight &l, float dist, float cosine) { return pdf_a_to_w(quad_pdf_area(l), dist, cosine); }
__device__ __forceinline__ f3 quad_sample_point(const flx_arealight &l, uint32_t *seed)
{
    f3 posL = V(l.pos);
    const float r1 = 2.0f * rand01(seed) - 1.0f;
    const float r2 = 2.0f * rand01(seed) - 1.0f;
    posL = posL + r1 * l.size.x * V(l.right);
    posL = posL + r2 * l.size.y * V(l.up);
    return posL;
}
// lenScale: the wavefront integrator shortens the shadow ray by 0.995 and -- the reference's quirk -- puts the SHORTENED length into the pdf; the microkernel's is 1
__device__ __forceinline__ LightSample quad_sample(const flx_arealight &l, f3 orig, uint32_t *seed, float lenScale)
{
    LightSample s;
    s.L = quad_sample_point(l, seed) - orig;
    s.rayLen = length(s.L) * lenScale;
    s.L = normalize(s.L);
    s.cosLight = fmaxf_(dot(V(l.N), -s.L), 0.0f);
    s.pdfA = quad_pdf_area(l); s.pdfDist = s.rayLen;
    return s;
}

// ---- the lamps: the emissive triangles of the table `ml`.  Callers check lamps_pickable first: without a pickable light nothing is drawn.
__device__ __forceinline__ bool lamps_pickable(const MeshLights &ml) { return ml.n && ml.hdr[1] != ML_NONE; }
__device__ __forceinline__ float lamp_pdf_area(const MeshLights &ml, uint32_t k, f3 p0, f3 p1, f3 p2) { return flxml::ml_pdf_area(ml.pick[k], flxml::ml_area(p0, p1, p2)); }
__device__ __forceinline__ float lamp_pdf_w(const MeshLights &ml, uint32_t k, f3 p0, f3 p1, f3 p2, float dist, float cosine) { return pdf_a_to_w(lamp_pdf_area(ml, k, p0, p1, p2), dist, cosine); }
// three draws (pick, r1, r2).  The TRUE distance enters the pdf; the shadow ray stops short of the lamp, which is in the tree (the reference's factor for its own light)
__device__ __forceinline__ LightSample lamp_sample(const Scene &sc, const MeshLights &ml, f3 orig, uint32_t *seed, uint32_t *tri)
{
    const float pk = rand01(seed);
    const float r1 = rand01(seed);
    const float r2 = rand01(seed);
    const uint32_t k = flxml::ml_pick(ml.cdf, ml.n, ml.hdr[1], pk);
    *tri = ml.tri[k];
    f3 p0, p1, p2;
    ml_vertices(sc, *tri, &p0, &p1, &p2);
    LightSample s;
    s.L = flxml::ml_sample_triangle(p0, p1, p2, r1, r2) - orig;
    const float lenL = length(s.L);
    s.L = normalize(s.L);
    s.rayLen = 0.995f * lenL;
    s.cosLight = fmaxf_(dot(flxml::ml_normal(p0, p1, p2), -s.L), 0.0f);
    s.pdfA = lamp_pdf_area(ml, k, p0, p1, p2); s.pdfDist = lenL;
    return s;
}
// An implicit hit on triangle `tri`: false unless its material emits, the hit counts (as an environment hit does) and the ray sees the side the geometric
// normal faces; then *Ke is what it emits and *misWeight its weight against lamp_sample's pdf x kindProb.  lastSpecular(), hitPoint() and kindProb() are
// called only where their value is needed -- the callers' loads behind them stay as lazy as they were.
template <class LastSpecular, class HitPoint, class KindProb>
__device__ __forceinline__ bool lamp_implicit(const Scene &sc, const flx_render_params &p, const MeshLights &ml, int tri, int matId, uint32_t len, f3 rayOrig, f3 rayDir,
                                              float lastPdfW, LastSpecular lastSpecular, HitPoint hitPoint, KindProb kindProb, f3 *Ke, float *misWeight)
{
    *Ke = V(sc.materials[matId].Ke);
    if (!(flxml::ml_is_emissive(Ke->x, Ke->y, Ke->z) && (len == 1u || p.sampleImpl))) return false;
    f3 p0, p1, p2;
    ml_vertices(sc, (uint32_t)tri, &p0, &p1, &p2);
    const f3 ng = flxml::ml_normal(p0, p1, p2);
    if (!(dot(ng, rayDir) < 0.0f)) return false;
    *misWeight = 1.0f;
    const bool spec = lastSpecular();
    if (p.sampleExpl && len > 1u && !spec && lamps_pickable(ml)) {
        const uint32_t k = flxml::ml_find(ml.tri, ml.n, (uint32_t)tri);
        if (k != ML_NONE)                                            // a light too small to be picked has pdf 0: weight 1 (flx_mesh_light.h)
            *misWeight = mis_implicit(lastPdfW, lamp_pdf_w(ml, k, p0, p1, p2, length(hitPoint() - rayOrig), dot(normalize(-rayDir), ng)), kindProb());
    }
    return true;
}

// ---- the wavefront integrator's ONE kind draw: the probability of each kind of light, from the parameters and whether the lamps are a kind (lamps_pickable)
struct KindProbs { bool lamps; float env, quad, lamp, envOrQuad; };     // envOrQuad: the kind draw below which the kind is not the lamps
__device__ __forceinline__ KindProbs light_kind_probs(uint32_t useEnvMap, uint32_t useAreaLight, bool lampsKind)
{
    uint32_t den = useEnvMap + useAreaLight + (lampsKind ? 1u : 0u); if (den < 1u) den = 1u;
    KindProbs k;
    k.lamps = lampsKind;
    k.env = (float)useEnvMap / (float)den;
    k.quad = lampsKind ? (float)useAreaLight / (float)den : 1.0f - k.env;
    k.lamp = 1.0f / (float)den;
    k.envOrQuad = (float)(useEnvMap + useAreaLight) / (float)den;
    return k;
}

} // namespace flxd
