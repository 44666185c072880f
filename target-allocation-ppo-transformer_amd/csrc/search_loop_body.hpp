// search_loop_body.hpp -- the loop of phases, scans and exchanges of the exchange searches, as
// statements: included INSIDE the body of k_search (search.hip), of k_search_constrained
// (search_constrained.hip) and of k_search_multistart (search_multistart.hip), once each, so that all
// three run one text. (As a function on RefineRow the loop compiled to different code in
// k_search_constrained, by reference and by value alike; this form leaves that object byte for byte
// what it was.)
// Reads r (RefineRow, after load_columns and, with LIM, start_limits), lane, max_exchanges, max_sweeps;
// defines exchanges and scan_clean (1: the last scan found no improving pair).
int exchanges = 0, scan_clean = 0;
for (;;) {
    r.phase(max_sweeps);
    if (max_exchanges == 0) break;
    double bd;
    int bi, bj;
    best_exchange(r, bd, bi, bj);
    if (!(bd > 0.0)) {
        scan_clean = 1;
        break;
    }
    if (exchanges == max_exchanges) break;
    const int ai = readlane_i(r.a, bi), aj = readlane_i(r.a, bj);
    if (lane == bi) r.a = aj;
    if (lane == bj) r.a = ai;
    ++exchanges;
}
