// dw_products_dump.cpp -- csrc/dw_products.h as JSON, for tests/test_dw_products_cpu.py (plain C++, no GPU, no HIP).
//
//   dw_products_dump < requests > out.json
//
// Always printed: "products" (the 14 rows; each operand with its kind, layer and width in both storage forms) and "split"
// (GRAD_BUCKET_SPLIT).  Requests on stdin, one per line:
//   plan <bf16|e4m3> <bucket> <cus> <P>     -> an entry of "plans": dw_plan's result
//   scratch <P>                             -> an entry of "scratch": the offsets inside the e4m3 scratch and its size
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "dw_products.h"

using namespace nerf_layout;

static void print_operand(const char* name, DwOperand o) {
    static const char* const kinds[] = {"DY", "ACT", "POSX", "POSD", "DSR"};
    std::printf("\"%s\": {\"kind\": \"%s\", \"layer\": %d, \"width\": {\"bf16\": %d, \"e4m3\": %d}}", name, kinds[(int)o.kind], o.layer,
                dw_operand_width(o, DW_BF16), dw_operand_width(o, DW_E4M3));
}

static void print_ints(const char* name, const int* v, int n) {
    std::printf("\"%s\": [", name);
    for (int i = 0; i < n; ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("]");
}

int main() {
    std::printf("{\"split\": %d,\n\"products\": [\n", GRAD_BUCKET_SPLIT);
    for (int i = 0; i < DW_NUM_PRODUCTS; ++i) {
        const DwProduct& p = DW_PRODUCTS[i];
        std::printf("  {");
        print_operand("a", p.a);
        std::printf(", ");
        print_operand("b", p.b);
        std::printf(", \"coff\": %d, \"ldc\": %d, \"r0\": %d, \"Mv\": %d, \"Nv\": %d, \"boff\": %d}%s\n", p.coff, p.ldc, p.r0, p.Mv, p.Nv,
                    p.boff, i + 1 < DW_NUM_PRODUCTS ? "," : "");
    }
    std::printf("],\n\"plans\": [\n");
    int plans = 0;
    std::vector<std::string> scratch;
    std::string what;
    while (std::cin >> what) {
        if (what == "plan") {
            std::string form;
            int bucket, cus;
            long long P;
            if (!(std::cin >> form >> bucket >> cus >> P) || (form != "bf16" && form != "e4m3")) return 2;
            const DwPlan plan = dw_plan(form == "bf16" ? DW_BF16 : DW_E4M3, P, bucket, cus);
            std::printf("%s  {\"form\": \"%s\", \"bucket\": %d, \"cus\": %d, \"P\": %lld, \"n\": %d, \"workgroups\": %d, ",
                        plans++ ? ",\n" : "", form.c_str(), bucket, cus, P, plan.n, plan.workgroups);
            print_ints("product", plan.product, plan.n);
            std::printf(", ");
            print_ints("wg0", plan.wg0, plan.n);
            std::printf(", ");
            print_ints("wgs", plan.wgs, plan.n);
            std::printf("}");
        } else if (what == "scratch") {
            long long P;
            if (!(std::cin >> P)) return 2;
            const F8Scratch s = f8_scratch(P);
            char line[256];
            std::snprintf(line, sizeof line, "  {\"P\": %lld, \"px\": %lld, \"pd\": %lld, \"ds\": %lld, \"total\": %lld}", P, s.px, s.pd, s.ds, s.total);
            scratch.push_back(line);
        } else {
            return 2;
        }
    }
    std::printf("\n],\n\"scratch\": [\n");
    for (size_t i = 0; i < scratch.size(); ++i) std::printf("%s%s\n", scratch[i].c_str(), i + 1 < scratch.size() ? "," : "");
    std::printf("]}\n");
    return 0;
}
