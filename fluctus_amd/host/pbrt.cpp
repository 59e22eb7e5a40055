// pbrt.cpp -- PBRT (v3 text format) scene ingest: Scene::loadPBRTModel.  SURVEY 8(f) N1.
//
// The reference reads .pbrt through the third-party ingowald/pbrt-parser (git submodule ext/pbrt-parser, unpinned and EMPTY
// in the reference checkout): .pbrt -> that library's binary .pbf cache -> pbrt::Scene -> Scene::loadPBFModel
// (reference: src/scene.cpp:53-103, 574-813).  The library is absent, so this file parses the published pbrt-v3 input
// format itself (https://pbrt.org/fileformat-v3) and applies the reference's OWN mapping from the parsed scene to its
// triangle / material arrays, which is all the wavefront path ever sees:
//   * geometry: trianglemesh and plymesh shapes; spheres, disks, curves, quads are skipped as in the reference (:676-693);
//     object instancing flattened, instance transform x shape transform applied to P, inverse-transpose to N (:659-660),
//     flat normal when the mesh has none (:667-668); world shapes first, then the instances in file order (:598-699);
//   * materials numbered in order of first use, 0 = the default material (:606-618); matte -> diffuse; plastic, substrate,
//     uber -> glossy; glass -> ideal dielectric; mirror -> ideal reflection; metal -> GGX reflection; roughness remap
//     (1 - r) * 5000 (:722-726, :729-806); image textures through the same lookup as the OBJ path (:711-720);
//   * world-up from the camera frame (:703-705).
// PARITY UNPINNED: no .pbrt/.pbf asset, test or golden vector exists in the reference checkout and the parser library is
// missing, so this loader is checked against hand-built scenes only (tests/test_host.py), not against the reference.
#include "scene.hpp"
#include "texture.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>

namespace fluctus {
namespace {

struct V3 { float x = 0, y = 0, z = 0; };
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 normalize(V3 a) { float l = std::sqrt(dot(a, a)); float inv = l > 0 ? 1.0f / l : 0.0f; return {a.x * inv, a.y * inv, a.z * inv}; }
inline flx_vec3 W(V3 v) { return flx_vec3{v.x, v.y, v.z, 0.0f}; }

struct M4 {                                      // row-major 4x4, points are column vectors
    float m[4][4];
    static M4 identity() { M4 r; memset(r.m, 0, sizeof(r.m)); for (int i = 0; i < 4; i++) r.m[i][i] = 1.0f; return r; }
    M4 operator*(const M4 &b) const
    {
        M4 r;
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { float s = 0; for (int k = 0; k < 4; k++) s += m[i][k] * b.m[k][j]; r.m[i][j] = s; }
        return r;
    }
    V3 point(V3 p) const { return {m[0][0] * p.x + m[0][1] * p.y + m[0][2] * p.z + m[0][3], m[1][0] * p.x + m[1][1] * p.y + m[1][2] * p.z + m[1][3], m[2][0] * p.x + m[2][1] * p.y + m[2][2] * p.z + m[2][3]}; }
    // inverse transpose of the linear part applied to a normal; not re-normalised (the reference does not either)
    V3 normal(V3 n) const
    {
        const float a = m[0][0], b = m[0][1], c = m[0][2], d = m[1][0], e = m[1][1], f = m[1][2], g = m[2][0], h = m[2][1], i = m[2][2];
        const float det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
        const float id = det != 0.0f ? 1.0f / det : 0.0f;
        // cofactor matrix / det = inverse transpose
        return {((e * i - f * h) * n.x + (f * g - d * i) * n.y + (d * h - e * g) * n.z) * id,
                ((c * h - b * i) * n.x + (a * i - c * g) * n.y + (b * g - a * h) * n.z) * id,
                ((b * f - c * e) * n.x + (c * d - a * f) * n.y + (a * e - b * d) * n.z) * id};
    }
    M4 inverse() const                            // general 4x4 (Gauss-Jordan); singular -> identity
    {
        float a[4][8];
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { a[i][j] = m[i][j]; a[i][j + 4] = i == j ? 1.0f : 0.0f; }
        for (int c = 0; c < 4; c++) {
            int piv = c;
            for (int r = c + 1; r < 4; r++) if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
            if (a[piv][c] == 0.0f) return identity();
            if (piv != c) for (int j = 0; j < 8; j++) std::swap(a[piv][j], a[c][j]);
            const float inv = 1.0f / a[c][c];
            for (int j = 0; j < 8; j++) a[c][j] *= inv;
            for (int r = 0; r < 4; r++) if (r != c) { const float f = a[r][c]; if (f != 0.0f) for (int j = 0; j < 8; j++) a[r][j] -= f * a[c][j]; }
        }
        M4 r; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.m[i][j] = a[i][j + 4];
        return r;
    }
};

// ---- tokens: numbers / identifiers, "quoted strings", [ and ]; # comments
struct Token { enum Kind { End, Word, String, LBracket, RBracket } kind = End; std::string text; };

struct Lexer {
    std::string src, file; size_t pos = 0; int line = 1;
    Token next()
    {
        for (;;) {
            while (pos < src.size() && isspace((unsigned char)src[pos])) { if (src[pos] == '\n') line++; pos++; }
            if (pos < src.size() && src[pos] == '#') { while (pos < src.size() && src[pos] != '\n') pos++; continue; }
            break;
        }
        Token t;
        if (pos >= src.size()) return t;
        const char c = src[pos];
        if (c == '[') { pos++; t.kind = Token::LBracket; return t; }
        if (c == ']') { pos++; t.kind = Token::RBracket; return t; }
        if (c == '"') {
            size_t e = src.find('"', pos + 1);
            if (e == std::string::npos) throw std::runtime_error(file + ": unterminated string at line " + std::to_string(line));
            t.kind = Token::String; t.text = src.substr(pos + 1, e - pos - 1); pos = e + 1; return t;
        }
        size_t e = pos;
        while (e < src.size() && !isspace((unsigned char)src[e]) && src[e] != '[' && src[e] != ']' && src[e] != '"' && src[e] != '#') e++;
        t.kind = Token::Word; t.text = src.substr(pos, e - pos); pos = e; return t;
    }
};

struct Param { std::string type, name; std::vector<float> nums; std::vector<std::string> strs; };
struct Params {
    std::vector<Param> list;
    const Param *find(const std::string &name) const { for (const Param &p : list) if (p.name == name) return &p; return nullptr; }
    float f(const std::string &name, float def) const { const Param *p = find(name); return p && (p->type == "float" || p->type == "integer") && !p->nums.empty() ? p->nums[0] : def; }
    bool b(const std::string &name, bool def) const { const Param *p = find(name); return p && p->type == "bool" && !p->strs.empty() ? p->strs[0] == "true" : def; }
    std::string s(const std::string &name, const std::string &def) const { const Param *p = find(name); return p && p->type == "string" && !p->strs.empty() ? p->strs[0] : def; }
    // rgb / color triple; a spectrum given as numbers or as a file, and texture references, keep the default
    V3 rgb(const std::string &name, V3 def) const
    {
        const Param *p = find(name);
        if (p && (p->type == "rgb" || p->type == "color") && p->nums.size() >= 3) return {p->nums[0], p->nums[1], p->nums[2]};
        if (p && p->type == "float" && p->nums.size() == 1) return {p->nums[0], p->nums[0], p->nums[0]};
        return def;
    }
    std::string tex(const std::string &name) const { const Param *p = find(name); return p && p->type == "texture" && !p->strs.empty() ? p->strs[0] : std::string(); }
};

struct PMaterial { std::string type; Params params; V3 Ke{}; };         // Ke: the AreaLightSource the shape was made under (L * scale), else 0
typedef std::shared_ptr<PMaterial> MatRef;
struct PTexture { std::string cls, filename; };

struct Mesh {                                   // one trianglemesh / plymesh, object space
    std::vector<V3> P, N; std::vector<float> uv; std::vector<int> idx;
    M4 xform; MatRef material;
};
struct Instance { std::string object; M4 xform; };
struct Object { std::vector<Mesh> meshes; std::vector<Instance> instances; };

// areaLight: AreaLightSource "diffuse" is part of the attribute state, like the material (pbrt-v3 s. B.3.4): pushed and popped with it
struct GState { M4 ctm = M4::identity(); MatRef material; bool areaLight = false; V3 L{}; };

// ---- PLY (plymesh): ascii / binary_little_endian / binary_big_endian; x y z [nx ny nz] [u v | s t]; faces as index lists
void loadPlyMesh(const std::string &path, Mesh &mesh)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open " + path);
    struct Prop { std::string name, type, countType; bool list = false; };
    struct Elem { std::string name; size_t count = 0; std::vector<Prop> props; };
    std::vector<Elem> elems;
    std::string line, format;
    std::getline(in, line);
    if (line.compare(0, 3, "ply") != 0) throw std::runtime_error("not a PLY file: " + path);
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        std::istringstream ss(line); std::string w; ss >> w;
        if (w == "format") ss >> format;
        else if (w == "element") { Elem e; ss >> e.name >> e.count; elems.push_back(e); }
        else if (w == "property" && !elems.empty()) {
            Prop p; ss >> p.type;
            if (p.type == "list") { p.list = true; ss >> p.countType >> p.type; }
            ss >> p.name; elems.back().props.push_back(p);
        } else if (w == "end_header") break;
    }
    const bool ascii = format == "ascii", big = format == "binary_big_endian";
    if (!ascii && !big && format != "binary_little_endian") throw std::runtime_error("unsupported PLY format '" + format + "': " + path);
    auto typeSize = [](const std::string &t) -> int {
        if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
        if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
        if (t == "int" || t == "uint" || t == "float" || t == "int32" || t == "uint32" || t == "float32") return 4;
        if (t == "double" || t == "float64") return 8;
        return 0;
    };
    auto readNum = [&](const std::string &t) -> double {
        if (ascii) { double v = 0; in >> v; if (!in) throw std::runtime_error("truncated PLY: " + path); return v; }
        unsigned char b[8]; const int n = typeSize(t);
        if (!n) throw std::runtime_error("unknown PLY type '" + t + "': " + path);
        in.read((char *)b, n);
        if (!in) throw std::runtime_error("truncated PLY: " + path);
        if (big) for (int i = 0; i < n / 2; i++) std::swap(b[i], b[n - 1 - i]);
        if (t == "float" || t == "float32") { float v; memcpy(&v, b, 4); return v; }
        if (t == "double" || t == "float64") { double v; memcpy(&v, b, 8); return v; }
        if (t == "char" || t == "int8") return (signed char)b[0];
        if (t == "uchar" || t == "uint8") return b[0];
        if (t == "short" || t == "int16") { int16_t v; memcpy(&v, b, 2); return v; }
        if (t == "ushort" || t == "uint16") { uint16_t v; memcpy(&v, b, 2); return v; }
        if (t == "int" || t == "int32") { int32_t v; memcpy(&v, b, 4); return v; }
        uint32_t v; memcpy(&v, b, 4); return v;
    };
    for (const Elem &e : elems) {
        const bool isVertex = e.name == "vertex", isFace = e.name == "face";
        bool hasN = false, hasUV = false;
        for (const Prop &p : e.props) { if (p.name == "nx") hasN = true; if (p.name == "u" || p.name == "s") hasUV = true; }
        for (size_t i = 0; i < e.count; i++) {
            V3 pos, nrm; float u = 0, v = 0;
            for (const Prop &p : e.props) {
                if (p.list) {
                    const int n = (int)readNum(p.countType);
                    std::vector<int> ix((size_t)std::max(n, 0));
                    for (int k = 0; k < n; k++) ix[(size_t)k] = (int)readNum(p.type);
                    if (isFace && (p.name == "vertex_indices" || p.name == "vertex_index"))
                        for (int k = 2; k < n; k++) { mesh.idx.push_back(ix[0]); mesh.idx.push_back(ix[(size_t)k - 1]); mesh.idx.push_back(ix[(size_t)k]); }   // fan
                    continue;
                }
                const float val = (float)readNum(p.type);
                if (!isVertex) continue;
                if (p.name == "x") pos.x = val; else if (p.name == "y") pos.y = val; else if (p.name == "z") pos.z = val;
                else if (p.name == "nx") nrm.x = val; else if (p.name == "ny") nrm.y = val; else if (p.name == "nz") nrm.z = val;
                else if (p.name == "u" || p.name == "s") u = val; else if (p.name == "v" || p.name == "t") v = val;
            }
            if (isVertex) { mesh.P.push_back(pos); if (hasN) mesh.N.push_back(nrm); if (hasUV) { mesh.uv.push_back(u); mesh.uv.push_back(v); } }
        }
    }
}

struct Parser {
    Scene &scene;
    std::string folder;
    std::vector<GState> attrStack;
    std::vector<M4> xformStack;
    GState gs;
    std::map<std::string, M4> namedCS;
    std::map<std::string, MatRef> namedMaterials;
    std::map<std::string, PTexture> textures;
    std::map<std::string, Object> objects;
    Object world;
    Object *current = nullptr;                  // ObjectBegin .. ObjectEnd target, else the world
    bool haveCamera = false; M4 cameraToWorld = M4::identity();
    int includeDepth = 0;

    explicit Parser(Scene &s) : scene(s) {}

    static bool isDirective(const Token &t) { return t.kind == Token::Word && !t.text.empty() && isupper((unsigned char)t.text[0]); }

    // reads `"type name" value...` pairs until the next directive; leaves that token in `look`
    Params readParams(Lexer &lx, Token &look)
    {
        Params ps;
        look = lx.next();
        while (look.kind == Token::String) {
            Param p;
            std::istringstream ss(look.text); ss >> p.type >> p.name;
            if (p.name.empty()) throw std::runtime_error(lx.file + ": bad parameter declaration \"" + look.text + "\" at line " + std::to_string(lx.line));
            Token t = lx.next();
            auto take = [&](const Token &v) {
                if (v.kind == Token::String) p.strs.push_back(v.text);
                else if (v.kind == Token::Word) { if (v.text == "true" || v.text == "false") p.strs.push_back(v.text); else p.nums.push_back(strtof(v.text.c_str(), nullptr)); }
            };
            if (t.kind == Token::LBracket) { for (t = lx.next(); t.kind != Token::RBracket && t.kind != Token::End; t = lx.next()) take(t); }
            else take(t);
            ps.list.push_back(std::move(p));
            look = lx.next();
        }
        return ps;
    }

    void floats(Lexer &lx, float *out, int n)
    {
        Token t = lx.next();
        const bool bracket = t.kind == Token::LBracket;
        if (bracket) t = lx.next();
        for (int i = 0; i < n; i++) {
            if (t.kind != Token::Word) throw std::runtime_error(lx.file + ": expected a number at line " + std::to_string(lx.line));
            out[i] = strtof(t.text.c_str(), nullptr);
            if (i + 1 < n || bracket) t = lx.next();
        }
        if (bracket && t.kind != Token::RBracket) throw std::runtime_error(lx.file + ": expected ] at line " + std::to_string(lx.line));
    }

    // a copy of `base` (none: the default material's parameters) that emits Ke; one copy per (material, Ke), so a lamp of many shapes is one material
    struct Emissive { MatRef base; V3 Ke; MatRef copy; };
    std::vector<Emissive> emissives;
    MatRef emissive(const MatRef &base, const V3 &Ke)
    {
        for (const Emissive &e : emissives) if (e.base == base && e.Ke.x == Ke.x && e.Ke.y == Ke.y && e.Ke.z == Ke.z) return e.copy;
        auto m = std::make_shared<PMaterial>();
        if (base) *m = *base; else m->type = "default";
        m->Ke = Ke;
        emissives.push_back({base, Ke, m});
        return m;
    }

    void addShape(const std::string &type, const Params &ps)
    {
        Mesh mesh; mesh.xform = gs.ctm; mesh.material = gs.areaLight ? emissive(gs.material, gs.L) : gs.material;
        if (type == "trianglemesh") {
            const Param *P = ps.find("P"), *I = ps.find("indices"), *N = ps.find("N"), *UV = ps.find("uv");
            if (!UV) UV = ps.find("st");
            if (!P || P->nums.size() % 3) throw std::runtime_error("trianglemesh without a valid \"point P\"");
            for (size_t i = 0; i + 2 < P->nums.size(); i += 3) mesh.P.push_back({P->nums[i], P->nums[i + 1], P->nums[i + 2]});
            if (N && N->nums.size() == P->nums.size()) for (size_t i = 0; i + 2 < N->nums.size(); i += 3) mesh.N.push_back({N->nums[i], N->nums[i + 1], N->nums[i + 2]});
            if (UV && UV->nums.size() / 2 == mesh.P.size()) mesh.uv = UV->nums;
            if (I) for (float v : I->nums) mesh.idx.push_back((int)v);
            else if (mesh.P.size() == 3) { mesh.idx = {0, 1, 2}; }
        } else if (type == "plymesh") {
            const std::string fn = ps.s("filename", "");
            if (fn.empty()) throw std::runtime_error("plymesh without \"string filename\"");
            loadPlyMesh(folder + fn, mesh);
        } else return;                               // sphere, disk, curve, ...: skipped like the reference (:676-693)
        if (mesh.idx.size() % 3) mesh.idx.resize(mesh.idx.size() / 3 * 3);
        (current ? current : &world)->meshes.push_back(std::move(mesh));
    }

    void parseFile(const std::string &path)
    {
        if (++includeDepth > 32) throw std::runtime_error("PBRT Include nesting too deep");
        std::ifstream in(path, std::ios::binary);
        if (!in) throw std::runtime_error("cannot open " + path);
        Lexer lx; lx.file = path;
        { std::ostringstream ss; ss << in.rdbuf(); lx.src = ss.str(); }
        Token t = lx.next();
        while (t.kind != Token::End) {
            if (!isDirective(t)) throw std::runtime_error(path + ": unexpected token '" + t.text + "' at line " + std::to_string(lx.line));
            const std::string d = t.text;
            Token look; bool haveLook = false;
            float v[16];
            if (d == "Identity") gs.ctm = M4::identity();
            else if (d == "Translate") { floats(lx, v, 3); M4 m = M4::identity(); m.m[0][3] = v[0]; m.m[1][3] = v[1]; m.m[2][3] = v[2]; gs.ctm = gs.ctm * m; }
            else if (d == "Scale") { floats(lx, v, 3); M4 m = M4::identity(); m.m[0][0] = v[0]; m.m[1][1] = v[1]; m.m[2][2] = v[2]; gs.ctm = gs.ctm * m; }
            else if (d == "Rotate") {
                floats(lx, v, 4);
                const V3 a = normalize({v[1], v[2], v[3]});
                const float th = v[0] * 3.14159265358979323846f / 180.0f, s = std::sin(th), c = std::cos(th);
                M4 m = M4::identity();
                m.m[0][0] = a.x * a.x + (1 - a.x * a.x) * c; m.m[0][1] = a.x * a.y * (1 - c) - a.z * s; m.m[0][2] = a.x * a.z * (1 - c) + a.y * s;
                m.m[1][0] = a.x * a.y * (1 - c) + a.z * s; m.m[1][1] = a.y * a.y + (1 - a.y * a.y) * c; m.m[1][2] = a.y * a.z * (1 - c) - a.x * s;
                m.m[2][0] = a.x * a.z * (1 - c) - a.y * s; m.m[2][1] = a.y * a.z * (1 - c) + a.x * s; m.m[2][2] = a.z * a.z + (1 - a.z * a.z) * c;
                gs.ctm = gs.ctm * m;
            } else if (d == "LookAt") {
                floats(lx, v, 9);
                const V3 eye{v[0], v[1], v[2]}, dir = normalize(V3{v[3], v[4], v[5]} - eye), up{v[6], v[7], v[8]};
                const V3 right = normalize(cross(normalize(up), dir)), newUp = cross(dir, right);
                M4 c2w = M4::identity();
                c2w.m[0][0] = right.x; c2w.m[1][0] = right.y; c2w.m[2][0] = right.z;
                c2w.m[0][1] = newUp.x; c2w.m[1][1] = newUp.y; c2w.m[2][1] = newUp.z;
                c2w.m[0][2] = dir.x; c2w.m[1][2] = dir.y; c2w.m[2][2] = dir.z;
                c2w.m[0][3] = eye.x; c2w.m[1][3] = eye.y; c2w.m[2][3] = eye.z;
                gs.ctm = gs.ctm * c2w.inverse();
            } else if (d == "Transform" || d == "ConcatTransform") {
                floats(lx, v, 16);
                M4 m; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) m.m[i][j] = v[j * 4 + i];      // the file lists columns
                gs.ctm = d == "Transform" ? m : gs.ctm * m;
            } else if (d == "CoordinateSystem") { Token n = lx.next(); namedCS[n.text] = gs.ctm; }
            else if (d == "CoordSysTransform") { Token n = lx.next(); auto it = namedCS.find(n.text); if (it != namedCS.end()) gs.ctm = it->second; }
            else if (d == "ReverseOrientation" || d == "WorldEnd") {}
            else if (d == "WorldBegin") { gs.ctm = M4::identity(); namedCS["world"] = gs.ctm; }
            else if (d == "AttributeBegin") attrStack.push_back(gs);
            else if (d == "AttributeEnd") { if (attrStack.empty()) throw std::runtime_error(path + ": unmatched AttributeEnd"); gs = attrStack.back(); attrStack.pop_back(); }
            else if (d == "TransformBegin") xformStack.push_back(gs.ctm);
            else if (d == "TransformEnd") { if (xformStack.empty()) throw std::runtime_error(path + ": unmatched TransformEnd"); gs.ctm = xformStack.back(); xformStack.pop_back(); }
            else if (d == "ObjectBegin") { Token n = lx.next(); attrStack.push_back(gs); current = &objects[n.text]; }
            else if (d == "ObjectEnd") { current = nullptr; if (!attrStack.empty()) { gs = attrStack.back(); attrStack.pop_back(); } }
            else if (d == "ObjectInstance") { Token n = lx.next(); (current ? current : &world)->instances.push_back({n.text, gs.ctm}); }
            else if (d == "Include") { Token n = lx.next(); parseFile(folder + n.text); }
            else if (d == "NamedMaterial") { Token n = lx.next(); auto it = namedMaterials.find(n.text); gs.material = it != namedMaterials.end() ? it->second : MatRef(); }
            else if (d == "MakeNamedMaterial") {
                Token n = lx.next(); Params ps = readParams(lx, look); haveLook = true;
                auto m = std::make_shared<PMaterial>(); m->type = ps.s("type", "matte"); m->params = std::move(ps);
                namedMaterials[n.text] = m;
            } else if (d == "Material") {
                Token n = lx.next(); Params ps = readParams(lx, look); haveLook = true;
                auto m = std::make_shared<PMaterial>(); m->type = n.text; m->params = std::move(ps);
                gs.material = m;
            } else if (d == "Texture") {
                Token name = lx.next(), type = lx.next(), cls = lx.next();
                Params ps = readParams(lx, look); haveLook = true;
                (void)type;
                textures[name.text] = PTexture{cls.text, ps.s("filename", "")};
            } else if (d == "Shape") {
                Token n = lx.next(); Params ps = readParams(lx, look); haveLook = true;
                addShape(n.text, ps);
            } else if (d == "Camera") {
                Token n = lx.next(); Params ps = readParams(lx, look); haveLook = true;
                (void)n; (void)ps;
                if (!haveCamera) { cameraToWorld = gs.ctm.inverse(); haveCamera = true; }
                namedCS["camera"] = cameraToWorld;
            } else if (d == "AreaLightSource") {
                // "diffuse" with "rgb L" / "color L" (default 1 1 1) and an optional "float scale": the shapes made under it emit Ke = L * scale
                // on the side their geometric normal faces (option "mesh_lights").  "twosided" is IGNORED: lamps are one-sided.
                Token n = lx.next(); Params ps = readParams(lx, look); haveLook = true;
                if (n.text == "diffuse" || n.text == "area") {
                    const V3 L = ps.rgb("L", {1.0f, 1.0f, 1.0f}); const float sc = ps.f("scale", 1.0f);
                    gs.areaLight = true; gs.L = {L.x * sc, L.y * sc, L.z * sc};
                }
            } else if (d == "MediumInterface") { Token a = lx.next(); look = lx.next(); if (look.kind == Token::String) look = lx.next(); haveLook = true; (void)a; }
            else {
                // Film, Sampler, Integrator, PixelFilter, Accelerator, LightSource, MakeNamedMedium, ...:
                // one type string + a parameter list, none of which reaches the triangle / material arrays
                Token n = lx.next(); (void)n;
                (void)readParams(lx, look); haveLook = true;
            }
            t = haveLook ? look : lx.next();
        }
        includeDepth--;
    }

    // ---- the reference's conversion (src/scene.cpp:598-813)
    std::vector<MatRef> usedMaterials;

    void emit(const Object &obj, const M4 &xform, int depth)
    {
        if (depth > 64) throw std::runtime_error("PBRT object instancing too deep (cycle?)");
        for (const Mesh &mesh : obj.meshes) {
            int matId = 0;
            if (mesh.material) {
                size_t k = 0;
                while (k < usedMaterials.size() && usedMaterials[k] != mesh.material) k++;
                if (k == usedMaterials.size()) usedMaterials.push_back(mesh.material);
                matId = (int)k + 1;
            }
            const M4 full = xform * mesh.xform;
            const bool hasN = !mesh.N.empty(), hasUV = !mesh.uv.empty();
            const int nv = (int)mesh.P.size();
            for (size_t i = 0; i + 2 < mesh.idx.size(); i += 3) {
                V3 p[3], n[3], t[3];
                bool ok = true;
                for (int k = 0; k < 3; k++) {
                    int ix = mesh.idx[i + (size_t)k];
                    if (ix < 0) ix += (int)(mesh.idx.size() / 3);           // the reference's handling of negative indices (:640-644)
                    if (ix < 0 || ix >= nv) { ok = false; break; }
                    p[k] = full.point(mesh.P[(size_t)ix]);
                    n[k] = hasN && (size_t)ix < mesh.N.size() ? full.normal(mesh.N[(size_t)ix]) : V3{};
                    t[k] = hasUV ? V3{mesh.uv[2 * (size_t)ix], mesh.uv[2 * (size_t)ix + 1], 0.0f} : V3{};
                }
                if (!ok) continue;                                            // out-of-range index: the reference reads past the array
                if (!hasN) n[0] = n[1] = n[2] = normalize(cross(p[1] - p[0], p[2] - p[0]));
                flx_triangle tri; memset(&tri, 0, sizeof(tri));
                tri.v0.p = W(p[0]); tri.v1.p = W(p[1]); tri.v2.p = W(p[2]);
                tri.v0.n = W(n[0]); tri.v1.n = W(n[1]); tri.v2.n = W(n[2]);
                tri.v0.t = W(t[0]); tri.v1.t = W(t[1]); tri.v2.t = W(t[2]);
                tri.matId = matId;
                scene.getTriangles().push_back(tri);
            }
        }
        for (const Instance &inst : obj.instances) {
            auto it = objects.find(inst.object);
            if (it != objects.end()) emit(it->second, xform * inst.xform, depth + 1);
        }
    }

    int loadTex(const std::string &texName)
    {
        if (texName.empty()) return -1;
        auto it = textures.find(texName);
        if (it == textures.end() || it->second.cls != "imagemap" || it->second.filename.empty()) return -1;     // "Unsupported texture type"
        return scene.tryImportTexture(folder + it->second.filename, it->second.filename);
    }

    void convertMaterials()
    {
        // pbrt-v3 accepts any roughness; outside [0, 1] the remap would give Ns < 0 (to_roughness NaN / inf: every path through the material NaN)
        auto rough = [](float r, bool remap, float ru, float rv) { const float res = std::min(1.0f, std::max(0.0f, r > 0.0f ? r : 0.5f * (ru + rv)));
                                                                  return (1.0f - res) * (remap ? 5000.0f : 1.0f); };
        for (const MatRef &pm : usedMaterials) {
            flx_material m = scene.getMaterials()[0];                        // default parameters (:732)
            const Params &ps = pm->params;
            const std::string &ty = pm->type;
            if (ty == "plastic") {
                m.type = FLX_BXDF_GLOSSY; m.Kd = W(ps.rgb("Kd", {0.25f, 0.25f, 0.25f})); m.Ks = W(ps.rgb("Ks", {0.25f, 0.25f, 0.25f}));
                m.Ns = rough(ps.f("roughness", 0.1f), ps.b("remaproughness", true), 0.0f, 0.0f);
                m.map_Kd = loadTex(ps.tex("Kd")); m.map_Ks = loadTex(ps.tex("Ks")); m.Ni = 1.5f;
            } else if (ty == "matte" || ty.empty()) {
                m.type = FLX_BXDF_DIFFUSE; m.Kd = W(ps.rgb("Kd", {0.5f, 0.5f, 0.5f})); m.map_Kd = loadTex(ps.tex("Kd"));
            } else if (ty == "substrate") {
                m.type = FLX_BXDF_GLOSSY; m.Kd = W(ps.rgb("Kd", {0.5f, 0.5f, 0.5f})); m.Ks = W(ps.rgb("Ks", {0.5f, 0.5f, 0.5f}));
                m.Ns = rough(0.0f, ps.b("remaproughness", true), ps.f("uroughness", 0.1f), ps.f("vroughness", 0.1f));
                m.map_Kd = loadTex(ps.tex("Kd")); m.map_Ks = loadTex(ps.tex("Ks")); m.Ni = 1.5f;
            } else if (ty == "uber") {
                m.type = FLX_BXDF_GLOSSY; m.Kd = W(ps.rgb("Kd", {0.25f, 0.25f, 0.25f})); m.Ks = W(ps.rgb("Ks", {0.25f, 0.25f, 0.25f}));
                m.Ns = rough(ps.f("roughness", 0.1f), true, ps.f("uroughness", 0.0f), ps.f("vroughness", 0.0f));
                m.map_Kd = loadTex(ps.tex("Kd")); m.map_Ks = loadTex(ps.tex("Ks")); m.Ni = ps.f("index", ps.f("eta", 1.5f));
            } else if (ty == "glass") {
                m.type = FLX_BXDF_IDEAL_DIELECTRIC; m.Ks = W(ps.rgb("Kt", {1.0f, 1.0f, 1.0f}));      // Ks = transmissivity
                const float ior = ps.f("index", ps.f("eta", 1.5f)); m.Ni = ior > 0.0f ? ior : 1.5f;
            } else if (ty == "mirror") {
                m.type = FLX_BXDF_IDEAL_REFLECTION; m.Ks = W(ps.rgb("Kr", {0.9f, 0.9f, 0.9f}));
            } else if (ty == "metal") {
                m.type = FLX_BXDF_GGX_ROUGH_REFLECTION;
                const V3 eta = ps.rgb("eta", {1.0f, 1.0f, 1.0f});                               // spectrum files keep the default
                m.Ni = (eta.x + eta.y + eta.z) / 3.0f; m.Ks = W(ps.rgb("k", {1.0f, 1.0f, 1.0f}));
                m.Ns = rough(ps.f("roughness", 0.01f), ps.b("remaproughness", true), ps.f("uroughness", 0.0f), ps.f("vroughness", 0.0f));
            }                                                                                  // fourier, hair, ...: default material (:807-818)
            m.Ke = W(pm->Ke);
            scene.addMaterial(m);
        }
    }
};

} // namespace

void Scene::loadPBRTModel(const std::string &filename)
{
    Parser ps(*this);
    size_t slash = filename.find_last_of("/\\");
    ps.folder = slash == std::string::npos ? std::string() : filename.substr(0, slash + 1);
    ps.parseFile(filename);
    ps.emit(ps.world, M4::identity(), 0);
    if (triangles.empty()) throw std::runtime_error("PBRT scene without triangle meshes: " + filename);
    // world up from the camera frame's y axis (src/scene.cpp:703-705); a scene without a camera keeps +Y
    if (ps.haveCamera) {
        const float vy = ps.cameraToWorld.m[1][1], vz = ps.cameraToWorld.m[2][1];
        worldUp = std::fabs(vy) > std::fabs(vz) ? flx_vec3{0.0f, 1.0f, 0.0f, 0.0f} : flx_vec3{0.0f, 0.0f, 1.0f, 0.0f};
    }
    ps.convertMaterials();
}

} // namespace fluctus
