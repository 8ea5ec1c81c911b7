// The host side of an audit of plan pieces (include/armour_hip.h, armour_path_audit*): the argument checks of the pieces, their sub-interval
// offsets, the merge words, the device round trip and the per-piece results.  Shared by path_audit.hip (against worlds) and self_check.hip
// (against the arm itself); host code only, nothing here is seen by a kernel.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "path_pieces.h"

namespace rmgeo {

// the piece arguments of an audit entry, as the caller passed them
struct PieceArgs {
    int32_t P;
    const double *q0, *qd0, *qdd0, *k, *k_range;
    double duration;
    const double *ta, *tb, *tube;
    double step;
};

inline void fill_pieces(int n, const PieceArgs& a, PaPieces* pc) {
    std::memset(pc, 0, sizeof(*pc));
    pc->q0 = a.q0; pc->qd0 = a.qd0; pc->qdd0 = a.qdd0; pc->k = a.k; pc->ta = a.ta; pc->tb = a.tb; pc->tube = a.tube;
    for (int j = 0; j < n; j++) pc->k_range[j] = a.k_range[j];
    pc->duration = a.duration;
    pc->step = a.step;
}

// The rules every audit entry holds its pieces to (n = the factors of a robot whose shape has been checked), then *pc = the pieces, host pointers.
inline int check_pieces(const char* who, int n, const PieceArgs& a, const int32_t* verdict, PaPieces* pc) {
    const int32_t P = a.P;
    if (!a.k_range || P < 0 || (P > 0 && (!a.q0 || !a.qd0 || !a.qdd0 || !a.k || !a.ta || !a.tb || !verdict))) {
        armour_set_error("%s: null argument", who);
        return ARMOUR_EINVAL;
    }
    if (!(a.step > 0.0) || !std::isfinite(a.step) || !(a.duration > 0.0) || !std::isfinite(a.duration)) {
        armour_set_error("%s: step = %g, duration = %g (both must be positive)", who, a.step, a.duration);
        return ARMOUR_EINVAL;
    }
    const size_t pn = (size_t)P * n;
    if (!finite_all(a.k_range, n) || !finite_all(a.q0, pn) || !finite_all(a.qd0, pn) || !finite_all(a.qdd0, pn) || !finite_all(a.k, pn) ||
        (a.tube && !finite_all(a.tube, pn))) {
        armour_set_error("%s: non-finite input", who);
        return ARMOUR_EINVAL;
    }
    for (int p = 0; p < P; p++) {
        if (!(a.ta[p] >= 0.0) || !(a.tb[p] >= a.ta[p]) || !(a.tb[p] <= a.duration)) {
            armour_set_error("%s: piece %d has the window [%g, %g], need 0 <= ta <= tb <= duration = %g", who, p, a.ta[p], a.tb[p], a.duration);
            return ARMOUR_EINVAL;
        }
        for (int j = 0; a.tube && j < n; j++)
            if (!(a.tube[(size_t)p * n + j] >= 0.0)) { armour_set_error("%s: piece %d has a negative tube radius", who, p); return ARMOUR_EINVAL; }
    }
    fill_pieces(n, a, pc);
    return ARMOUR_OK;
}

// piece_off [P + 1] of pieces that are in device order already: piece i owns items [piece_off[i], piece_off[i + 1])
inline int piece_offsets(const char* who, const RmRobot& rb, const PaPieces& pc, int32_t P, std::vector<int64_t>* piece_off) {
    piece_off->assign((size_t)P + 1, 0);
    for (int i = 0; i < P; i++) {
        const double S = piece_intervals(rb, pc, i);
        if (!(S + (double)(*piece_off)[i] <= (double)(INT32_MAX - 1))) {
            armour_set_error("%s: more than 2^31 - 2 (piece, sub-interval) items (step %g too small)", who, pc.step);
            return ARMOUR_ECAPACITY;
        }
        (*piece_off)[i + 1] = (*piece_off)[i] + (int64_t)S;
    }
    return ARMOUR_OK;
}

// What the items of an audit leave, on the host: per piece the merge words as audit_record expects them, per item `values` clearances.
struct AuditMerge {
    std::vector<int32_t> first_hit;
    std::vector<uint8_t> undecided;
    std::vector<double> item_clear;       // [items][values], empty in verdict mode
    AuditMerge(int32_t P, size_t clears) : first_hit(P, PA_NO_HIT), undecided(P, 0), item_clear(clears) {}
};

// The per-piece results from what the items left.  Piece i of pc / piece_off / mg is the caller's piece order[i] (order null: i itself);
// an item holds `values` clearances.
inline void finish_pieces(const PaPieces& pc, const std::vector<int64_t>& piece_off, const int32_t* order, int values, int32_t P, const AuditMerge& mg,
                          int32_t* verdict, double* t_hit, double* clearance) {
    for (int i = 0; i < P; i++) {
        const int p = order ? order[i] : i;
        const int64_t S = piece_off[i + 1] - piece_off[i];
        const int32_t first_hit = mg.first_hit[i];
        const bool hit = first_hit != PA_NO_HIT;
        verdict[p] = hit ? 1 : mg.undecided[i] ? 2 : 0;
        if (t_hit) {
            const double ta = pc.ta[i], w = pc.tb[i] - ta;
            t_hit[p] = hit ? ta + ((double)(2 * (int64_t)first_hit + 1) * w) / (double)(2 * S) : NAN;
        }
        if (clearance) {
            double cl = INFINITY;
            for (int64_t x = piece_off[i] * values; x < piece_off[i + 1] * values; x++) cl = fmin(cl, mg.item_clear[x]);
            clearance[p] = cl;
        }
    }
}

// The device copies of an audit's pieces and merge words, with the stream and the timing events of the one launch between upload and
// download: the caller adds what its kernel reads besides (on `st`), records ev's start and launches.
struct AuditDevice {
    DevStream st;
    EventPair ev;
    DevBuf<double> q0, qd0, qdd0, k, ta, tb, tube, clear;
    DevBuf<int32_t> item_piece, first_hit;
    DevBuf<int64_t> piece_off;
    DevBuf<uint8_t> undecided;
    std::vector<int32_t> host_item_piece;   // (read by its copy until download has synchronised)

    // *dev = pc with device pointers; the clearances (mg.item_clear's size) are only reserved
    int upload(const PaPieces& pc, int32_t P, int n, const std::vector<int64_t>& off, const AuditMerge& mg, PaPieces* dev) {
        host_item_piece.resize((size_t)off[P]);
        for (int i = 0; i < P; i++)
            for (int64_t x = off[i]; x < off[i + 1]; x++) host_item_piece[(size_t)x] = i;
        ARMOUR_TRY(st.create());
        const size_t pn = (size_t)P * n;
        ARMOUR_TRY(q0.upload(pc.q0, pn, st));
        ARMOUR_TRY(qd0.upload(pc.qd0, pn, st));
        ARMOUR_TRY(qdd0.upload(pc.qdd0, pn, st));
        ARMOUR_TRY(k.upload(pc.k, pn, st));
        ARMOUR_TRY(ta.upload(pc.ta, P, st));
        ARMOUR_TRY(tb.upload(pc.tb, P, st));
        if (pc.tube) ARMOUR_TRY(tube.upload(pc.tube, pn, st));
        ARMOUR_TRY(item_piece.upload(host_item_piece.data(), host_item_piece.size(), st));
        ARMOUR_TRY(piece_off.upload(off.data(), off.size(), st));
        ARMOUR_TRY(first_hit.upload(mg.first_hit.data(), P, st));
        ARMOUR_TRY(undecided.upload(mg.undecided.data(), P, st));
        if (!mg.item_clear.empty()) ARMOUR_TRY(clear.reserve(mg.item_clear.size()));
        *dev = pc;
        dev->q0 = q0; dev->qd0 = qd0; dev->qdd0 = qdd0; dev->k = k; dev->ta = ta; dev->tb = tb;
        dev->tube = pc.tube ? tube.p : nullptr;
        return ARMOUR_OK;
    }
    // after the launch: ev's stop, the merge words and clearances back, the stream synchronised; *ms (if given) = the time between the events
    int download(AuditMerge* mg, double* ms) {
        ARMOUR_TRY(ev.record_stop(st));
        const size_t P = mg->first_hit.size();
        HIPCHK(hipMemcpyAsync(mg->first_hit.data(), first_hit, P * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(mg->undecided.data(), undecided, P, hipMemcpyDeviceToHost, st));
        if (!mg->item_clear.empty()) HIPCHK(hipMemcpyAsync(mg->item_clear.data(), clear, mg->item_clear.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (ms) ARMOUR_TRY(ev.elapsed_ms(ms));
        return ARMOUR_OK;
    }
};

}  // namespace rmgeo
