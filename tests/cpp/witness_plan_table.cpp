// The table of record kinds of ezkl_amd/csrc/witness_plan.hpp, and the constants Python has twins of, printed one per line:
// tests/test_witness_plan_table.py compares them with ezkl_amd/witness_plan.py line for line.
#include <stdio.h>

#include "witness_plan.hpp"

using namespace ezkl::wplan;

int main() {
    static const char* const roles[] = {"cells", "indices", "digits", "words", "not a pool offset"};
    for (uint32_t kind = 0; kind < KINDS_TOP; kind++) {
        const KindInfo& K = KINDS[kind];
        printf("%u|%s|%s|%s|%d|%d|%s|%s|%d|%llu\n", kind, kind_name(kind), K.failure ? K.failure : "-", K.unit, (int)K.scan, (int)K.sparse, roles[K.a], roles[K.b], (int)known(kind),
               (unsigned long long)dst_words(kind, 3, 5));
    }
    printf("SORT_TILE=%u\nMAX_SORT_COUNT=%u\nARGEXT_CHUNK=%u\nSCATTER_TILE=%u\nMAX_PHASES=%u\nMAX_CHALLENGES=%u\nMAGIC=%u\nVERSION=%u\nKINDS_TOP=%u\nNONE=%u\n", SORT_TILE, MAX_SORT_COUNT,
           ARGEXT_CHUNK, SCATTER_TILE, MAX_PHASES, MAX_CHALLENGES, MAGIC, VERSION, (uint32_t)KINDS_TOP, NONE);
    return 0;
}
