// gen/codegen_body.cpp — the Body expression emitter (codegen_ctx.h): pool nodes as HIP
// expressions, one local temporary per node and kernel body.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "codegen_ctx.h"

namespace optamd {
namespace gen {

std::string lit(double v) {
    // (builtins: the runtime compiler's headers define neither HUGE_VAL nor NAN)
    if (std::isinf(v)) return v < 0 ? "(-(T)__builtin_huge_val())" : "((T)__builtin_huge_val())";
    if (std::isnan(v)) return "((T)__builtin_nan(\"\"))";
    char b[64];
    snprintf(b, sizeof(b), "%.17g", v);
    std::string s = b;
    if (s.find_first_of(".eEn") == std::string::npos) s += ".0";
    return "((T)" + s + ")";
}

const char* elem_type(const std::string& e, bool unknown) {
    if (unknown) return "T";
    if (e == "uint8") return "unsigned char";
    if (e == "int") return "int";
    return "float";
}

static bool transcendental(const Node& n) {
    switch (n.op) {
        case Op::Sin: case Op::Cos: case Op::Exp: case Op::Log: case Op::Sqrt:
        case Op::Tan: case Op::Tanh: case Op::Sinh: case Op::Cosh: case Op::Asin: case Op::Acos:
        case Op::Atan: case Op::Asinh: case Op::Acosh: case Op::Log10: return true;
        default: return false;
    }
}
bool cacheable(const Pool& P, const Node& n, bool slot) {
    if (!transcendental(n)) return false;
    const Node c = P.at(n.a);
    return c.op == Op::Read && (c.slot >= 0) == slot;
}

bool pred_form(const Pool& P, const Node& n, int* rd, double* c, bool* left) {
    if (n.op != Op::Lt && n.op != Op::Le && n.op != Op::Gt && n.op != Op::Ge && n.op != Op::Eq && n.op != Op::Ne) return false;
    if (P.is_const(n.b, c) && P.at(n.a).op == Op::Read) { *left = true; *rd = n.a; }
    else if (P.is_const(n.a, c) && P.at(n.b).op == Op::Read) { *left = false; *rd = n.b; }
    else return false;
    return P.at(*rd).slot < 0;
}
int pred_bit(const Ctx& ctx, const Node& n, int* rd) {
    double c;
    bool left;
    if (ctx.pred.keys.empty() || !pred_form(ctx.P, n, rd, &c, &left)) return -1;
    const Node& r = ctx.P.at(*rd);
    for (size_t k = 0; k < ctx.pred.keys.size(); ++k)
        if (ctx.pred.keys[k] == std::make_tuple((int)n.op, r.i, r.ch, c, left)) return (int)k;
    return -1;
}

bool Body::invariant(int id) {
    if (!pre_) return false;
    auto it = inv_.find(id);
    if (it != inv_.end()) return it->second;
    const Node n = P_.at(id);
    bool r = true;
    switch (n.op) {
        case Op::Const: case Op::Param: r = true; break;
        case Op::Read: r = n.slot == self_ && (n.g < 0 || n.g == graph_); break;
        case Op::InBox: case Op::Coord: case Op::Sample: case Op::Weight: r = false; break;
        default:
            r = (n.a < 0 || invariant(n.a)) && (n.b < 0 || invariant(n.b)) && (n.d < 0 || invariant(n.d));
    }
    inv_[id] = r;
    return r;
}

std::string Body::v(int id) {
    auto it = done_.find(id);
    if (it != done_.end()) return it->second;
    const Node n = P_.at(id);
    const GraphCache* gc = nullptr;
    if (!C_.gcache.empty() && cacheable(P_, n, true)) {
        auto gi = C_.gcache.find(M_.images[P_.at(n.a).i].space);
        if (gi != C_.gcache.end()) gc = &gi->second;
    }
    if (gc) {
        const Node c = P_.at(n.a);
        auto ci = gc->ch.find(std::make_tuple((int)n.op, c.i, c.ch));
        if (ci != gc->ch.end()) {
            const int W = gc->width, k = ci->second;
            const std::string rec = "((const T*)a.img[" + std::to_string(gc->img) + "]) + (long long)v" +
                                    std::to_string(c.slot) + " * " + std::to_string(W);
            const std::string rec32 = "opt_g32((const T*)a.img[" + std::to_string(gc->img) + "], v" +
                                      std::to_string(c.slot) + ", " + std::to_string(W) + ", ";
            std::string name;
            // the slot's whole record once as 16-byte vectors (per-edge kernels: gen_cost
            // 51.7 -> 41.5 us on 1M-vertex ARAP); the vertex gathers read the fields they use
            // (their edge loops: 83.8 us scalar, 90.0 us as records)
            if (W >= 4 && !pre_) {
                const std::string kr = "kr" + std::to_string(c.slot);
                if (!rec_.count(c.slot)) {
                    for (int g = 0; g < W; g += 4)
                        out(id) << "        const OptV4 " << kr << "_" << g / 4 << " = *(const OptV4*)(" << rec << " + "
                                << g << ");\n";
                    rec_.insert(c.slot);
                }
                name = kr + "_" + std::to_string(k / 4) + "." + "xyzw"[k % 4];
            } else {
                name = "k" + std::to_string(id);
                if (C_.off32 && W <= 16)  // (the plan's size check assumes <= 16 fields)
                    out(id) << "        const T " << name << " = " << rec32 << k << ");\n";
                else
                    out(id) << "        const T " << name << " = (" << rec << ")[" << k << "];\n";
            }
            done_[id] = name;
            return name;
        }
    }
    if (use_cache_ && !C_.cache.empty() && cacheable(P_, n, false)) {
        const Node c = P_.at(n.a);
        auto ci = C_.cache.find(std::make_tuple((int)n.op, c.i, c.ch));
        if (ci != C_.cache.end()) {
            // outside the image the argument reads 0: f(0), as the evaluated form
            const double f0 = fold1(n.op, 0.0);
            const std::string name = "k" + std::to_string(id);
            o_ << "        const T " << name << " = (" << inb(c.off) << ") ? ((const T*)a.img[" << ci->second
               << "])[li + " << rel(c.off) << "] : " << lit(f0) << ";\n";
            done_[id] = name;
            return name;
        }
    }
    std::string e;
    if (n.op != Op::Const && is_bool(id)) {   // a 0 / 1 value: its bool, as a number
        e = "(T)(" + bv(id) + ")";
        const std::string name = "t" + std::to_string(id);
        out(id) << "        const T " << name << " = " << e << ";\n";
        done_[id] = name;
        return name;
    }
    switch (n.op) {
        case Op::Const: done_[id] = lit(n.c); return done_[id];
        case Op::Param: e = "(T)a.prm[" + std::to_string(n.i) + "]"; break;
        case Op::Read: e = read(n, nullptr); break;
        case Op::Weight:
            if (!weight_) {
                fprintf(stderr, "[opt_amd] codegen: a loss group's weight in a kernel that has no place to read it\n");
                abort();
            }
            e = weight_(n.i);
            break;
        case Op::Coord: e = "(T)(" + std::string(1, "xyz"[n.i]) + " + " + std::to_string(n.off[n.i]) + ")"; break;
        case Op::Add: e = v(n.a) + " + " + v(n.b); break;
        case Op::Sub: e = v(n.a) + " - " + v(n.b); break;
        case Op::Mul: e = v(n.a) + " * " + v(n.b); break;
        case Op::Div: e = v(n.a) + " / " + v(n.b); break;
        case Op::Neg: e = "-" + v(n.a); break;
        case Op::Sqrt: e = "sqrt(" + v(n.a) + ")"; break;
        case Op::Sin:
        case Op::Cos: {   // one sincos per angle: both halves share the range reduction
            const std::string x = v(n.a), sn = "s" + std::to_string(n.a), cn = "c" + std::to_string(n.a);
            if (!sincos_.count(n.a)) {
                out(n.a) << "        T " << sn << ", " << cn << "; opt_sincos(" << x << ", &" << sn << ", &" << cn << ");\n";
                sincos_.insert(n.a);
            }
            done_[id] = n.op == Op::Sin ? sn : cn;
            return done_[id];
        }
        case Op::Exp: e = "exp(" + v(n.a) + ")"; break;
        case Op::Log: e = "log(" + v(n.a) + ")"; break;
        case Op::Abs: e = "fabs(" + v(n.a) + ")"; break;
        case Op::Pow: e = "pow(" + v(n.a) + ", " + v(n.b) + ")"; break;
        // overloaded on T: the float module calls the float versions
        case Op::Tan: e = "tan(" + v(n.a) + ")"; break;
        case Op::Tanh: e = "tanh(" + v(n.a) + ")"; break;
        case Op::Sinh: e = "sinh(" + v(n.a) + ")"; break;
        case Op::Cosh: e = "cosh(" + v(n.a) + ")"; break;
        case Op::Asin: e = "asin(" + v(n.a) + ")"; break;
        case Op::Acos: e = "acos(" + v(n.a) + ")"; break;
        case Op::Atan: e = "atan(" + v(n.a) + ")"; break;
        case Op::Asinh: e = "asinh(" + v(n.a) + ")"; break;
        case Op::Acosh: e = "acosh(" + v(n.a) + ")"; break;
        case Op::Log10: e = "log10(" + v(n.a) + ")"; break;
        case Op::Atan2: e = "atan2(" + v(n.a) + ", " + v(n.b) + ")"; break;
        case Op::Select: e = cond(n.a) + " ? " + v(n.b) + " : " + v(n.d); break;
        case Op::Sample:
            e = "opt_sample(" + img_ptr(n.i) + ", " + std::to_string(M_.images[n.i].channels) + ", " +
                std::to_string(n.ch) + ", " + v(n.a) + ", " + v(n.b) + ", W, H)";
            break;
        default: break;   // InBox, comparisons, And / Or / Not: boolean-valued, emitted above
    }
    const std::string name = "t" + std::to_string(id);
    out(id) << "        const T " << name << " = " << e << ";\n";
    done_[id] = name;
    return name;
}
// Boolean-valued nodes — comparisons, And / Or / Not, InBox, products of booleans, the
// constants 0 and 1 — are emitted as `bool` and turned into T only where a number is
// needed: the energies' validity masks (inside * (Mask == 0) * ...) become one && chain
// instead of float compares, conversions and multiplies, and a Select reads them directly
// (the same 0 / 1 values: a product of 0 / 1 numbers is their logical and).
bool Body::is_bool(int id) {
    auto it = isb_.find(id);
    if (it != isb_.end()) return it->second;
    const Node n = P_.at(id);
    bool r = false;
    switch (n.op) {
        case Op::Lt: case Op::Le: case Op::Gt: case Op::Ge: case Op::Eq: case Op::Ne:
        case Op::And: case Op::Or: case Op::Not: case Op::InBox: r = true; break;
        case Op::Const: r = n.c == 0.0 || n.c == 1.0; break;
        case Op::Mul: r = is_bool(n.a) && is_bool(n.b); break;
        default: r = false;
    }
    isb_[id] = r;
    return r;
}
std::string Body::bv(int id) {
    auto it = bdone_.find(id);
    if (it != bdone_.end()) return it->second;
    const Node n = P_.at(id);
    std::string e;
    int rd = -1;
    const int k = use_pred_ ? pred_bit(C_, n, &rd) : -1;
    if (k >= 0) {
        const int pr = P_.read(C_.pred.img, 0, P_.at(rd).off);
        const std::string w = read(P_.at(pr), nullptr);
        e = "((((int)(" + w + ")) >> " + std::to_string(k) + ") & 1) " + (C_.pred.at0[k] ? "== 0" : "!= 0");
        const std::string name = "b" + std::to_string(id);
        out(id) << "        const bool " << name << " = " << e << ";\n";
        bdone_[id] = name;
        return name;
    }
    switch (n.op) {
        case Op::Const: bdone_[id] = n.c != 0.0 ? "true" : "false"; return bdone_[id];
        case Op::Lt: e = v(n.a) + " < " + v(n.b); break;
        case Op::Le: e = v(n.a) + " <= " + v(n.b); break;
        case Op::Gt: e = v(n.a) + " > " + v(n.b); break;
        case Op::Ge: e = v(n.a) + " >= " + v(n.b); break;
        case Op::Eq: e = v(n.a) + " == " + v(n.b); break;
        case Op::Ne: e = v(n.a) + " != " + v(n.b); break;
        case Op::And: case Op::Mul: e = cond(n.a) + " && " + cond(n.b); break;
        case Op::Or: e = cond(n.a) + " || " + cond(n.b); break;
        case Op::Not: e = "!" + cond(n.a); break;
        case Op::InBox: e = inbox(n.off, n.off2); break;
        default: e = "false";
    }
    const std::string name = "b" + std::to_string(id);
    out(id) << "        const bool " << name << " = " << e << ";\n";
    bdone_[id] = name;
    return name;
}
std::string Body::vec(int u, const char* vname) {
    const std::string key = std::string(vname) + std::to_string(u);
    auto it = vdone_.find(key);
    if (it != vdone_.end()) return it->second;
    const Node n = P_.at(u);
    const std::string name = std::string(vname) + "_" + std::to_string(u);
    out(u) << "        const T " << name << " = " << read(n, vname) << ";\n";
    vdone_[key] = name;
    return name;
}

std::string Body::coord(int k, int off) const {
    const char c = "xyz"[k];
    return off == 0 ? std::string(1, c) : "(" + std::string(1, c) + (off > 0 ? " + " : " - ") +
                                               std::to_string(off > 0 ? off : -off) + ")";
}
std::string Body::inb(const int* off) const {
    std::string s;
    for (int k = 0; k < nd_; ++k) {
        if (off[k] == 0) continue;   // the thread's own coordinate is always inside
        if (!s.empty()) s += " && ";
        const char* dim = k == 0 ? "W" : k == 1 ? "H" : "D";
        s += coord(k, off[k]) + " >= 0 && " + coord(k, off[k]) + " < " + dim;
    }
    return s.empty() ? "true" : s;
}
// offset of a centred access from the thread's pixel, in pixels (32-bit: the
// front end limits the index space, generic_accepts)
std::string Body::rel(const int* off) const {
    std::string r = std::to_string(off[0]);
    if (nd_ > 1 && off[1]) r += " + " + std::to_string(off[1]) + " * W";
    if (nd_ > 2 && off[2]) r += " + " + std::to_string(off[2]) + " * W * H";
    return "(" + r + ")";
}
std::string Body::img_ptr(int i) const {
    const GImage& im = M_.images[i];
    return "((const " + std::string(elem_type(im.elem, im.tvalued)) + "*)a.img[" + std::to_string(i) + "])";
}
std::string Body::read(const Node& n, const char* vname) {
    const GImage& im = M_.images[n.i];
    const std::string ch = std::to_string(im.channels), c = std::to_string(n.ch);
    std::string base, idx;
    if (vname && C_.vec_base) {
        base = C_.vec_base(n.i, vname);
    } else if (vname) {
        base = std::string(vname) + " + a.uoff[" + std::to_string(C_.uslot[n.i]) + "]";
    } else {
        base = img_ptr(n.i);
    }
    if (n.slot >= 0) {
        if (C_.off32) return "(T)opt_g32(" + base + ", v" + std::to_string(n.slot) + ", " + ch + ", " + c + ")";
        idx = "(long long)v" + std::to_string(n.slot) + " * " + ch + " + " + c;
        return "(T)(" + base + ")[" + idx + "]";
    }
    if (centred_) return centred_(n, vname);
    idx ="(li + " + rel(n.off) + ") * " + ch + " + " + c;
    return "opt_ldm(" + base + ", " + idx + ", " + inb(n.off) + ")";
}

}  // namespace gen
}  // namespace optamd
