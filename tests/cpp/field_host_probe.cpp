// field_host_probe.cpp -- the __host__ halves of Field<P> (csrc/field.hpp) on operand rows from a file.
//
// The host halves compute twiddles, vanishing inverses and Kate powers on every proof and are compiled nowhere on their own.  This
// program runs the radix-2^32 primitives of the device probe (csrc/fieldprobe.hip) through them: mul_portable, the host branches of
// mul, mul_inl and mul_lazy, redc, and the add / sub / lazy family.  tests/test_field_edge_ref.py builds it for the host only, with
// UndefinedBehaviorSanitizer, feeds it the operand lists of tests/field_edge_ref.py and compares every word with Python integers.
//
//   field_host_probe IN OUT
// IN:  one row per line, "<fr|fq>.<primitive> <operand> [<operand>]", an operand being 64 hex digits, most significant first
// OUT: one result per line in the same form
#include <stdio.h>
#include <string.h>
#include "../../ezkl_amd/csrc/field.hpp"

using namespace ezkl;

static bool parse(const char* s, fe_t* out) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 8; i++) {
        uint32_t w = 0;
        for (int k = 0; k < 8; k++) {
            const char ch = s[(7 - i) * 8 + k];
            uint32_t d;
            if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
            else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a' + 10);
            else return false;
            w = (w << 4) | d;
        }
        out->v[i] = w;
    }
    return true;
}

template <class F>
static bool apply(const char* prim, int nops, const fe_t& a, const fe_t& b, fe_t* r) {
    struct Op {
        const char* name;
        int arity;
        fe_t (*f1)(const fe_t&);
        fe_t (*f2)(const fe_t&, const fe_t&);
    };
    static const Op ops[] = {
        {"add", 2, nullptr, &F::add},           {"sub", 2, nullptr, &F::sub},           {"neg", 1, &F::neg, nullptr},
        {"dbl", 1, &F::dbl, nullptr},           {"reduce_once", 1, &F::reduce_once, nullptr},
        {"mul", 2, nullptr, &F::mul},           {"mul_inl", 2, nullptr, &F::mul_inl},   {"sqr", 1, &F::sqr, nullptr},
        {"mul_lazy", 2, nullptr, &F::mul_lazy}, {"redc", 1, &F::redc, nullptr},         {"from_mont", 1, &F::from_mont, nullptr},
        {"to_mont", 1, &F::to_mont, nullptr},   {"add_lazy", 2, nullptr, &F::add_lazy}, {"sub_lazy", 2, nullptr, &F::sub_lazy},
        {"reduce_2p", 1, &F::reduce_2p, nullptr}, {"inv", 1, &F::inv, nullptr},
    };
    for (const Op& o : ops)
        if (!strcmp(o.name, prim)) {
            if (o.arity != nops) return false;
            *r = o.arity == 1 ? o.f1(a) : o.f2(a, b);
            return true;
        }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "r");
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) {
        fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    char name[64], sa[80], sb[80];
    char line[256];
    size_t lineno = 0;
    while (fgets(line, sizeof line, in)) {
        lineno++;
        const int got = sscanf(line, "%63s %79s %79s", name, sa, sb);
        fe_t a, b = Fr::zero(), r;
        if (got < 2 || !parse(sa, &a) || (got == 3 && !parse(sb, &b))) {
            fprintf(stderr, "line %zu: malformed\n", lineno);
            return 1;
        }
        bool ok = false;
        if (!strncmp(name, "fr.", 3)) ok = apply<Fr>(name + 3, got - 1, a, b, &r);
        else if (!strncmp(name, "fq.", 3)) ok = apply<Fq>(name + 3, got - 1, a, b, &r);
        if (!ok) {
            fprintf(stderr, "line %zu: unknown primitive or wrong operand count: %s\n", lineno, name);
            return 1;
        }
        fprintf(out, "%s %08x%08x%08x%08x%08x%08x%08x%08x\n", name, r.v[7], r.v[6], r.v[5], r.v[4], r.v[3], r.v[2], r.v[1], r.v[0]);
    }
    fclose(in);
    return fclose(out) ? 1 : 0;
}
