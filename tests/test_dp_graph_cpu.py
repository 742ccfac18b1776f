"""The host logic of the data-parallel step replayed as hipGraph segments, without a GPU: where `trainer.plan_segments` cuts the backward
program, and the protocol of `trainer.run_or_replay_segments` (eager twice, every body captured at the third call, replayed afterwards, the eager
work between the segments exactly once per segment per call) with a capture that only records."""
import types

import pytest

from multi_task_breast_cancer_amd import trainer as T


def buckets_of(ready_ops):
    """Hand-made buckets in `st.buckets` order (from the end of the flat buffer to its start), 10 elements each."""
    n = len(ready_ops)
    return [T.Bucket(10 * (n - 1 - i), 10 * (n - i), r) for i, r in enumerate(ready_ops)]


def check_tiling(segs, n_buckets, n_ops):
    """The ranges tile [0, n_ops) in order; every bucket appears exactly once, in `st.buckets` order."""
    at = 0
    for first, count, _ in segs:
        assert first == at and count >= 0
        at += count
    assert at == n_ops
    assert [k for _, _, bks in segs for k in bks] == list(range(n_buckets))


@pytest.mark.parametrize("ready,n_ops,expected", [
    ([9], 10, [(0, 10, (0,))]),                                                                     # one bucket behind the last op
    ([4], 10, [(0, 5, (0,)), (5, 5, ())]),                                                          # ops behind the last bucket
    ([2, 5, 7, 9], 10, [(0, 3, (0,)), (3, 3, (1,)), (6, 2, (2,)), (8, 2, (3,))]),
    ([2, 5, 5, 9], 12, [(0, 3, (0,)), (3, 3, (1,)), (6, 0, (2,)), (6, 4, (3,)), (10, 2, ())]),      # two buckets ready at the same op
    ([5, 2, 8], 10, [(0, 6, (0,)), (6, 0, (1,)), (6, 3, (2,)), (9, 1, ())]),                        # a ready_op that has been passed already
    ([3, 40], 10, [(0, 4, (0,)), (4, 6, (1,))]),                                                    # a ready_op beyond the program's end
    ([40, 3], 10, [(0, 10, (0,)), (10, 0, (1,))]),
    ([0, 1, 2, 3, 4, 5, 6, 7], 9, [(i, 1, (i,)) for i in range(8)] + [(8, 1, ())]),
    ([1, 1, 3, 2, 6, 6, 6, 30], 8, [(0, 2, (0,)), (2, 0, (1,)), (2, 2, (2,)), (4, 0, (3,)), (4, 3, (4,)), (7, 0, (5,)), (7, 0, (6,)), (7, 1, (7,))]),
    ([-1, 2], 4, [(0, 0, (0,)), (0, 3, (1,)), (3, 1, ())]),                                         # nothing to wait for: an empty FIRST range
    ([], 5, [(0, 5, ())]),
])
def test_plan_segments_cuts_the_backward_program_behind_each_bucket(ready, n_ops, expected):
    segs = T.plan_segments(buckets_of(ready), n_ops)
    assert segs == expected
    check_tiling(segs, len(ready), n_ops)


def test_plan_segments_tiles_for_every_small_layout():
    import itertools
    for n_ops in (1, 3, 6):
        for nb in (1, 2, 3, 4):
            for ready in itertools.product(range(-1, n_ops + 2), repeat=nb):
                segs = T.plan_segments(buckets_of(ready), n_ops)
                check_tiling(segs, nb, n_ops)
                done = 0
                for (first, count, bks), r in zip(segs, ready):        # each bucket follows the ops it waits for, and no more than those
                    done = first + count
                    assert done >= min(n_ops, r + 1) and (count == 0 or done == min(n_ops, r + 1))


def test_plan_segments_is_what_the_eager_loop_did():
    """The loop `FusedTrainStep.run` held before the function existed, on the same inputs."""
    import random
    rng = random.Random(7)
    for _ in range(200):
        n_ops, nb = rng.randint(1, 40), rng.randint(1, 8)
        bk = buckets_of([rng.randint(-1, n_ops + 3) for _ in range(nb)])
        log, done = [], 0
        for i, b in enumerate(bk):
            upto = min(n_ops, b.ready_op + 1)
            if upto > done:
                log.append(("run", done, upto - done))
                done = upto
            log.append(("reduce", i))
        if done < n_ops:
            log.append(("run", done, n_ops - done))
        new = []
        for first, count, bks in T.plan_segments(bk, n_ops):
            if count:
                new.append(("run", first, count))
            new += [("reduce", k) for k in bks]
        assert new == log


class Recorder:
    """Stands in for the capture function: records which body it was given and -- a capture executes nothing -- does NOT run it; the graph it
    returns logs the body's name at every replay."""

    def __init__(self, log):
        self.log, self.captured = log, []

    def __call__(self, body):
        self.captured.append(body.name)
        rec = self

        class Graph:
            name = body.name
            replays = 0

            def replay(self):
                self.replays += 1
                rec.log.append(("replay", self.name))

        return Graph()


def make_bodies(log, n):
    bodies = []
    for i in range(n):
        def body(i=i):
            log.append(("eager", f"body{i}"))
        body.name = f"body{i}"
        bodies.append(body)
    return bodies


def test_segment_driver_runs_eager_twice_captures_all_bodies_once_then_replays():
    owner, other = types.SimpleNamespace(_graphs={}), types.SimpleNamespace(_graphs={})
    st = types.SimpleNamespace()
    log = []
    rec = Recorder(log)
    bodies = make_bodies(log, 4)
    between = lambda i: log.append(("between", i))
    quiesce = lambda: log.append(("quiesce",))

    def call(who=owner, key="k"):
        del log[:]
        T.run_or_replay_segments(who, st, key, bodies, between, capture=rec, quiesce=quiesce)
        return list(log)

    def sequence(how):
        return [x for i in range(4) for x in ((how, f"body{i}"), ("between", i))]

    for n in (1, 2):                                            # calls 1 and 2: eager, body0, between0, body1, between1, ...
        assert call() == sequence("eager")
        assert st._graph_ents[id(owner)] == ["k", n, None] and rec.captured == []
    assert owner._graphs[id(st)] is st._graph_ents[id(owner)]
    third = call()                                              # call 3: the communication stream is drained, EVERY body is captured, nothing runs
    assert third[0] == ("quiesce",) and third[1:] == sequence("replay")      # eager meanwhile -- then the same sequence, as replays
    assert rec.captured == ["body0", "body1", "body2", "body3"]
    ent = st._graph_ents[id(owner)]
    assert ent[:2] == ["k", 2] and isinstance(ent[2], T.SegmentGraphs) and len(ent[2]) == 4
    assert [g.name for g in ent[2].graphs] == rec.captured
    held = ent[2]
    for n in (4, 5):                                            # calls 4 and 5: replays only, no second capture, no second drain
        assert call() == sequence("replay")
        assert len(rec.captured) == 4 and st._graph_ents[id(owner)][2] is held
    assert [g.replays for g in held.graphs] == [3, 3, 3, 3]
    assert call(other) == sequence("eager")                     # a second owner on the same compiled step keeps an entry of its own
    assert st._graph_ents[id(other)] == ["k", 1, None] and st._graph_ents[id(owner)][2] is held
    assert other._graphs[id(st)] is st._graph_ents[id(other)] and owner._graphs[id(st)] is st._graph_ents[id(owner)]
    assert call(key="moved") == sequence("eager")               # a changed key drops the graphs and restarts the count
    assert st._graph_ents[id(owner)] == ["moved", 1, None] and owner._graphs[id(st)] is st._graph_ents[id(owner)]
    assert call(key="moved") == sequence("eager")
    assert call(key="moved")[1:] == sequence("replay") and len(rec.captured) == 8
    assert st._graph_ents[id(owner)][2] is not held and st._graph_ents[id(other)] == ["k", 1, None]


def test_segment_driver_defaults_to_the_thread_local_capture_of_the_single_graph_recipe(monkeypatch):
    """The default capture of the segments is `_capture` itself under torch's thread-local capture-error mode; `run_or_replay` keeps the global one."""
    import inspect
    seen = []
    monkeypatch.setattr(T, "_capture", lambda body, error_mode="global": seen.append((body, error_mode)) or "graph")
    body = lambda: None
    assert T._capture_segment(body) == "graph" and seen == [(body, "thread_local")]
    assert inspect.signature(T.run_or_replay_segments).parameters["capture"].default is T._capture_segment
    assert inspect.signature(T.run_or_replay).parameters["capture"].default is not T._capture_segment


def test_distributed_step_issues_the_planned_segments(monkeypatch):
    """`FusedTrainStep._dp_segments` on a stub step: the bodies are the front (with the first backward range), one per further non-empty range,
    and the update; a bucket with an empty range is reduced behind its predecessor; the ranges it reports are `plan_segments`'."""
    log = []

    class Program:
        def __init__(self, name, n=1):
            self.name, self.n = name, n

        def run(self, first=0, count=None):
            log.append((self.name, first, self.n - first if count is None else count))

    class Stream:
        def wait_event(self, ev):
            log.append(("wait", ev.k))

        def synchronize(self):
            log.append(("drain",))

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    class Event:
        made = 0

        def __init__(self):
            self.k = Event.made
            Event.made += 1

        def record(self, stream):
            log.append(("record", self.k))

    class Current:
        def wait_stream(self, s):
            log.append(("join",))

    bk = buckets_of([5, 2, 8])
    st = types.SimpleNamespace(programs={k: Program(k) for k in ("pack", "fwd", "loss")}, buckets=bk)
    st.programs["bwd"] = Program("bwd", 10)
    comm = Stream()
    step = types.SimpleNamespace(scaler=None, metrics=False, comm_stream=comm, model=types.SimpleNamespace(flat_g="g"))
    monkeypatch.setattr(T.torch.cuda, "Event", Event)
    monkeypatch.setattr(T.torch.cuda, "current_stream", lambda: Current())
    monkeypatch.setattr(T.torch.cuda, "stream", lambda s: s)
    monkeypatch.setattr(T, "allreduce_buckets", lambda flat, bks: log.append(("reduce", bk.index(bks[0]))))
    bodies, between, ranges = T.FusedTrainStep._dp_segments(step, st, lambda: log.append(("update",)))
    assert ranges == ((0, 6), (6, 0), (6, 3), (9, 1)) == tuple((f, c) for f, c, _ in T.plan_segments(bk, 10))
    assert len(bodies) == 4                                     # front + (6, 3) + (9, 1) + update: the empty range makes no body
    for i, body in enumerate(bodies):
        body()
        between(i)
    again = T.FusedTrainStep._dp_segments(step, st, lambda: None)
    assert Event.made == 3 and again[2] == ranges               # the events are made once per compiled step
    assert log == [("pack", 0, 1), ("fwd", 0, 1), ("loss", 0, 1), ("bwd", 0, 6),
                   ("record", 0), ("wait", 0), ("reduce", 0), ("record", 1), ("wait", 1), ("reduce", 1),
                   ("bwd", 6, 3), ("record", 2), ("wait", 2), ("reduce", 2),
                   ("bwd", 9, 1), ("join",), ("update",)]
