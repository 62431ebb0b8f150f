/*
 * rt_launch_order.h — every wait between a context's two render streams, in one module without HIP.
 *
 * A context renders on a main stream (0: its own stream, or the caller's after rt_set_stream) and a side stream (1).  A single
 * frame goes out as two half kernels, one per stream; fused launches alternate between the streams; the tile-order sort runs on
 * the stream of the launch that needs it.  This module decides where a launch runs (place) and issues its steps with the events
 * that order them (run).  It reaches the runtime only through a Backend: rt_context.hip's issues HIP events and kernels,
 * tests/test_launch_order.py's records what was issued and checks it against a happens-before model.
 *
 *   what                          who writes it                     rule
 *   non-render work (uploads,     the main stream, through          fork_side: the side stream's next kernel waits for FORK, recorded on
 *    resets, read-backs)           join()                           the main stream (needFork); join() makes the main stream wait for
 *                                                                   what the side stream holds (JOIN, sideDirty)
 *   tile order buffer b,          the sort, on the stream of the    begin_sort: the rewrite of b waits for b's last readers on the other
 *    key snapshot                  launch that needs it             stream (ORDER_RETIRE b) and, the sorts sharing one key snapshot, for
 *                                                                   the previous sort if that ran there; end_sort records SORT, marks the
 *                                                                   other stream (sortPending) and retires the buffer going out of use;
 *                                                                   before_order_read: a stream's next trace kernel waits for SORT once
 *   accumulation buffer           single-frame trace kernels        before_acc_write(s, whole): wait for the other stream's last whole-image
 *                                  (whole image, or one half of a   writer (ACC_FULL) and, if this kernel or that stream's last writer
 *                                  two-part frame), accumulate      covers the whole image, for its last writer of any kind (ACC_WRITER).
 *                                  kernels (whole image)            Halves of consecutive two-part frames need no wait: between two sorts a
 *                                                                   stream's half is the same set of pixels; end_sort therefore declares
 *                                                                   both last writers "whole".  after_acc_write records the events.
 *   staging slab, pixel records,  launches on that stream only      stream order (nothing here)
 *    tile counter of a stream
 *
 * The bookkeeping of the sort (sortPending, ORDER_RETIRE) follows the CONTEXT: whether it can use the side stream at all
 * (twoStreams), never the shape of one launch.  A launch that stays on the main stream still marks the side stream, which may hold
 * an earlier launch's readers and will hold later ones.
 */
#pragma once

#include "../../include/rt_abi.h"

namespace rt_order {

enum Event {
    FORK, JOIN, SORT,
    ORDER_RETIRE0, ORDER_RETIRE1, /* per order buffer */
    ACC_WRITER0, ACC_WRITER1,     /* per stream */
    ACC_FULL0, ACC_FULL1,         /* per stream */
    EVENT_COUNT
};

/* Everything the module asks of the runtime; each call returns an RT_* status. */
struct Backend {
    virtual int record(Event e, int stream) = 0;
    virtual int wait(int stream, Event e) = 0;
    virtual int sort(int stream, int target) = 0;             /* rewrite order buffer `target` from a snapshot of the tile costs */
    virtual int trace(int stream, int part, int parts) = 0;   /* the trace kernel of part `part` of `parts` */
    virtual int accumulate(int stream) = 0;                   /* add a fused launch's staged frames into the accumulation buffer */
protected:
    ~Backend() = default;
};

struct Shape {
    int frames = 1;          /* > 1: a fused launch (frames staged, then accumulated in frame order) */
    bool singleWave = true;  /* single-wave workgroups; pooled and group launches stay on the main stream */
    int tiles = 0;
};

struct Placement {
    int frames = 1;
    bool staged = false;     /* frames > 1 */
    bool split = false;      /* the launch may use the side stream */
    int lane = 0;            /* stream of a fused launch or a one-part frame */
    int parts = 1;           /* 2: the two halves of a single frame, part p on stream p */
    int sortTarget = -1;     /* order buffer the launch re-sorts before its trace, -1 = none */
    long long framesAfter = 0; /* frames rendered at this image size once the launch is issued (counted with the tile order only) */
};

#define RT_ORDER_TRY(call)               \
    do {                                 \
        const int rc_ = (call);          \
        if (rc_ != RT_OK) return rc_;    \
    } while (0)

class LaunchOrder {
public:
    /* the context can use the side stream: RT_TWO_STREAMS, on its own stream, the side stream exists */
    bool twoStreams = false;
    /* placement: fused launches alternate between the streams (off while the second slab does not fit, or RT_ALTERNATE=0) */
    bool alternate = true;
    int stagedNext = 0;               /* lane of the next fused launch */
    /* the tile order's schedule: re-sorted once 1, 2, 4, 8, ... frames have been rendered at this size (RT_LPT=0: never) */
    bool lpt = true;
    long long framesSinceResize = 0, nextSortAt = 1;
    int orderCur = 0;                 /* the order buffer traces read ... */
    bool orderValid = false;          /* ... once a sort has written one */
    /* cross-stream state (s = 0 main, 1 side) */
    bool sideDirty = false;           /* the side stream holds work the main stream has not been ordered after */
    bool needFork = true;             /* the main stream holds non-render work the side stream must follow */
    bool sortPending[2] = {false, false};  /* stream s has not been ordered after the last sort */
    bool retireValid[2] = {false, false};  /* ORDER_RETIRE b has been recorded since the buffers were made */
    /* the accumulation buffer is added to in launch order whichever stream a launch runs on: ACC_WRITER s marks the last kernel on
     * stream s that writes it; accWriterPending[s] = the other stream has not been ordered after it yet; accWriterFull[s] = that kernel
     * touches every pixel (false = one half of a two-part frame) */
    bool accWriterPending[2] = {false, false};
    bool accWriterFull[2] = {false, false};
    /* the last WHOLE-IMAGE writer of a stream is tracked on its own: a half kernel behind it on the same stream re-records ACC_WRITER
     * with full = false, and the other stream's half of that very frame would then no longer wait for the whole-image writer
     * (rt_render_frames(17): 16 fused frames + 1 two-part frame; found by tools/soak.py, round 4) */
    bool accFullPending[2] = {false, false};

    /* after a host synchronise (rt_create, rt_set_stream): nothing is in flight, nothing is pending */
    void set_two_streams(bool on)
    {
        twoStreams = on;
        sideDirty = false;
        needFork = true;
        for (int s = 0; s < 2; s++) sortPending[s] = retireValid[s] = accWriterPending[s] = accFullPending[s] = false;
    }

    /* the order buffers were re-made (another image size): nothing reads them, nothing is learnt yet */
    void forget_order()
    {
        sortPending[0] = sortPending[1] = false;
        retireValid[0] = retireValid[1] = false;
        orderValid = false;
        orderCur = 0;
        framesSinceResize = 0;
        nextSortAt = 1;
    }

    /* the main stream, ordered after everything the side stream has been given: every use of the main stream other than a render
     * launch goes through here */
    int join(Backend& b)
    {
        needFork = true;
        if (!sideDirty) return RT_OK;
        sideDirty = false;
        accWriterPending[1] = false; /* whatever the side stream adds to the accumulation buffer now precedes the main stream's next kernel */
        accFullPending[1] = false;
        RT_ORDER_TRY(b.record(JOIN, 1));
        return b.wait(0, JOIN);
    }

    Placement place(const Shape& shape) const
    {
        Placement p;
        p.frames = shape.frames;
        p.staged = shape.frames > 1;
        p.split = twoStreams && shape.singleWave;
        p.lane = p.staged && p.split && alternate ? stagedNext : 0;
        p.parts = !p.staged && p.split && shape.tiles >= 2 ? 2 : 1;
        if (lpt && framesSinceResize >= nextSortAt) p.sortTarget = orderValid ? 1 - orderCur : 0;
        p.framesAfter = framesSinceResize + (lpt ? shape.frames : 0);
        return p;
    }

    /* issue a placed launch: sort, trace kernel(s), accumulate, with the waits and records they need */
    int run(const Placement& p, Backend& b)
    {
        if (p.sortTarget >= 0) { /* a single frame's two halves: sorted on the main stream, the side stream waits */
            while (nextSortAt <= framesSinceResize) nextSortAt *= 2;
            RT_ORDER_TRY(begin_sort(b, p.lane, p.sortTarget));
            RT_ORDER_TRY(b.sort(p.lane, p.sortTarget));
            RT_ORDER_TRY(end_sort(b, p.lane, orderValid ? orderCur : -1));
            orderCur = p.sortTarget;
            orderValid = true;
        }
        framesSinceResize = p.framesAfter;
        if (p.parts == 2 || p.lane == 1) RT_ORDER_TRY(fork_side(b)); /* the side stream follows what the main stream holds so far */
        for (int part = 0; part < p.parts; part++) {
            const int s = p.parts == 2 ? part : p.lane;
            RT_ORDER_TRY(before_order_read(b, s));
            if (!p.staged) RT_ORDER_TRY(before_acc_write(b, s, p.parts == 1)); /* the trace kernel itself adds into the accumulation buffer */
            RT_ORDER_TRY(b.trace(s, part, p.parts));
            if (s == 1) sideDirty = true;
            if (!p.staged) RT_ORDER_TRY(after_acc_write(b, s, p.parts == 1));
        }
        if (!p.staged && p.parts == 1) accWriterPending[1] = false; /* ordered before the main stream's whole-image kernel just launched */
        if (p.staged) {
            /* the frames' colours were staged: added in frame order, after every earlier frame's */
            RT_ORDER_TRY(before_acc_write(b, p.lane, true));
            RT_ORDER_TRY(b.accumulate(p.lane));
            RT_ORDER_TRY(after_acc_write(b, p.lane, true));
            accWriterPending[1 - p.lane] = false; /* this accumulate is ordered after it; later writers wait for this one */
            if (p.split && alternate) stagedNext = 1 - p.lane;
        } else if (p.parts == 2) {
            /* a fused launch that follows a two-part frame goes behind the part that started first and ends first (the main stream's), so
             * its waves take the slots the other part's drain leaves empty instead of waiting for that drain to end */
            stagedNext = 0;
        }
        return RT_OK;
    }

private:
    int fork_side(Backend& b)
    {
        if (!needFork) return RT_OK;
        RT_ORDER_TRY(b.record(FORK, 0));
        RT_ORDER_TRY(b.wait(1, FORK));
        needFork = false;
        return RT_OK;
    }

    int begin_sort(Backend& b, int s, int target)
    {
        if (s == 1) RT_ORDER_TRY(fork_side(b));
        if (retireValid[target]) RT_ORDER_TRY(b.wait(s, Event(ORDER_RETIRE0 + target)));
        if (sortPending[s]) RT_ORDER_TRY(b.wait(s, SORT)); /* (two sorts in consecutive launches on alternating streams) */
        return RT_OK;
    }
    int end_sort(Backend& b, int s, int retiring /* buffer going out of use, or -1 */)
    {
        RT_ORDER_TRY(b.record(SORT, s));
        sortPending[s] = false;
        sortPending[1 - s] = twoStreams;
        if (retiring >= 0 && twoStreams) { /* whatever the other stream holds so far may still read it */
            RT_ORDER_TRY(b.record(Event(ORDER_RETIRE0 + retiring), 1 - s));
            retireValid[retiring] = true;
        }
        if (s == 1) sideDirty = true;
        /* a new order moves pixels between the two halves of a two-part frame: the next such frame's halves must come after BOTH
         * streams' last kernels that add into the accumulation buffer */
        accWriterFull[0] = accWriterFull[1] = true;
        return RT_OK;
    }
    int before_order_read(Backend& b, int s)
    {
        if (!sortPending[s]) return RT_OK;
        RT_ORDER_TRY(b.wait(s, SORT));
        sortPending[s] = false;
        return RT_OK;
    }

    int before_acc_write(Backend& b, int s, bool whole)
    {
        if (accFullPending[1 - s]) { /* once waited for, everything later on this stream follows it */
            RT_ORDER_TRY(b.wait(s, Event(ACC_FULL0 + 1 - s)));
            accFullPending[1 - s] = false;
        }
        if (accWriterPending[1 - s] && (whole || accWriterFull[1 - s])) RT_ORDER_TRY(b.wait(s, Event(ACC_WRITER0 + 1 - s)));
        return RT_OK;
    }
    int after_acc_write(Backend& b, int s, bool whole)
    {
        RT_ORDER_TRY(b.record(Event(ACC_WRITER0 + s), s));
        accWriterPending[s] = true;
        accWriterFull[s] = whole;
        if (whole) {
            RT_ORDER_TRY(b.record(Event(ACC_FULL0 + s), s));
            accFullPending[s] = true;
        }
        return RT_OK;
    }
};

} // namespace rt_order
