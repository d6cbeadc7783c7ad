"""SequenceDataReader through the C ABI (aslp_sequence_reader_*, include/aslp_nnet.h) on archives in Kaldi formats: every batch -- features,
labels, mask, new-utterance flags -- against a numpy restatement of the reference's stream bookkeeping (data-reader.cc:200-325), once
with the batches gathered on the device (the default) and once assembled on the host (aslp_stream_batch_on_host(1)); the two must agree bit
for bit, and with a feature transform the default must not wait for the device once between its first and its last read."""
import numpy as np
import pytest
import torch

import kaldi_formats as kf

pytestmark = pytest.mark.gpu

D, A, B = 7, 11, 5
TRANSFORM = """<NnetProto>
<Splice> <InputDim> %d <OutputDim> %d <BuildVector> -1:1 </BuildVector>
<AddShift> <InputDim> %d <OutputDim> %d <InitParam> 0.5
<Rescale> <InputDim> %d <OutputDim> %d <InitParam> 0.25
</NnetProto>
""" % (D, 3 * D, 3 * D, 3 * D, 3 * D, 3 * D)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """lengths 1, 2 (shorter than a delay of 2), 10 (a multiple of the batch size), random in 3..41; one utterance without targets (skipped);
    one with a soft frame (no label for that row)"""
    tmp = tmp_path_factory.mktemp("seqreader")
    rng = np.random.default_rng(5)
    lens = [7, 1, 10, 2] + [int(x) for x in rng.integers(3, 42, 4)]
    keys = ["q%02d" % i for i in range(len(lens))]
    feats = [rng.standard_normal((n, D)).astype(np.float32) for n in lens]
    posts = [[[(int(rng.integers(0, A)), 1.0)] for _ in range(n)] for n in lens]
    posts[6][1] = [(2, 0.5), (3, 0.5)]
    (tmp / "feats.ark").write_bytes(kf.archive([(k, kf.matrix_bin(f)) for k, f in zip(keys, feats)]))
    (tmp / "post.ark").write_bytes(kf.archive([(k, kf.posterior_bin(p)) for i, (k, p) in enumerate(zip(keys, posts)) if i != 4]))
    utts = [(f, [p[0][0] if len(p) == 1 else -1 for p in post]) for i, (f, post) in enumerate(zip(feats, posts)) if i != 4]
    return dict(feats="ark:%s" % (tmp / "feats.ark"), post="ark:%s" % (tmp / "post.ark"), utts=utts)


@pytest.fixture(autouse=True)
def switch_back(aslp):
    yield
    aslp.ops.stream_batch_on_host(-1)


def restate(utts, S, delay, w, off, cols):
    todo = list(utts)
    cur, length, which, flags = [0] * S, [0] * S, [None] * S, [0] * S
    x, lab, out = np.zeros((0, 0), np.float32), np.full(B * S, -1, np.int32), []
    while True:
        for s in range(S):
            if cur[s] < length[s]:
                flags[s] = 0
                continue
            if todo:
                f, l = todo.pop(0)
                idx = np.arange(off, len(f), w) if w > 1 else np.arange(len(f))
                which[s], cur[s], length[s], flags[s] = (f[idx], [l[i] for i in idx]), 0, len(idx), 1
        done = all(cur[s] >= length[s] for s in range(S))
        mask = np.zeros(B * S, np.float32)
        if not done:
            x = np.zeros((B * S, cols), np.float32)   # (rows of a stream without frames stay +0.0)
            lab = lab.copy()
            for t in range(B):
                for s in range(S):
                    r = t * S + s
                    if length[s] == 0:                # ... and the row keeps the target it had
                        cur[s] += 1
                        continue
                    f, l = which[s]
                    if cur[s] < length[s]:
                        mask[r] = 1.0
                        lab[r] = l[cur[s]]
                    else:
                        lab[r] = l[length[s] - 1]
                    x[r] = f[min(cur[s] + delay, length[s] - 1)]
                    cur[s] += 1
        out.append(dict(feat=x, labels=lab, mask=mask, flags=np.array(flags, np.int32)))
        if done and not todo:
            return out


def read_all(aslp, corpus, S, delay, w, off, transform):
    r = aslp.SequenceReader(corpus["feats"], corpus["post"], batch_size=B, num_stream=S, targets_delay=delay, skip_width=w, skip_offset=off,
                            transform=transform)
    got, syncs = [], []
    while not r.Done():
        syncs.append(aslp.ops.device_to_host_syncs())
        got.append(r.Read(num_pdf=A))
    syncs.append(aslp.ops.device_to_host_syncs())
    return got, syncs


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


CONFIGS = [(0, 1, 0), (2, 1, 0), (1, 2, 0), (1, 2, 1), (1, 3, 0), (1, 3, 1), (1, 3, 2)]


@pytest.mark.parametrize("with_transform", [False, True], ids=["raw", "transform"])
@pytest.mark.parametrize("delay,w,off", CONFIGS, ids=["delay%d-skip%d-off%d" % c for c in CONFIGS])
def test_batches_match_restatement_on_device_and_on_host(aslp, dev, corpus, delay, w, off, with_transform):
    n_utt = len(corpus["utts"])
    transform = aslp.Nnet.Init(TRANSFORM, seed=1) if with_transform else None
    utts = corpus["utts"]
    if with_transform:   # the transform's own arithmetic is not this test's subject: its output per utterance, through the API
        other = aslp.Nnet.Init(TRANSFORM, seed=1)
        utts = [(other.Feedforward(torch.from_numpy(f).to(dev)).cpu().numpy(), l) for f, l in utts]
    for S in (3, n_utt + 2):   # fewer streams than utterances, and more (streams that never receive one)
        want = restate(utts, S, delay, w, off, utts[0][0].shape[1])
        legs = {}
        for on_host in (0, 1):
            aslp.ops.stream_batch_on_host(on_host)
            got, syncs = read_all(aslp, corpus, S, delay, w, off, transform)
            assert len(got) == len(want) and len(got) > 3
            for i, (g, e) in enumerate(zip(got, want)):
                where = (S, on_host, i)
                assert np.array_equal(bits(g["feat"].cpu().numpy()), bits(e["feat"])), where
                assert np.array_equal(g["labels_host"], e["labels"]) and np.array_equal(g["labels"].cpu().numpy(), e["labels"]), where
                assert np.array_equal(g["mask_host"], e["mask"]) and np.array_equal(g["mask"].cpu().numpy(), e["mask"]), where
                assert np.array_equal(g["new_utt_flags"], e["flags"]), where
                assert g["one_hot"] == bool((e["labels"] >= 0).all()) and g["done"] == (i == len(want) - 1), where
            legs[on_host] = got
            if with_transform:
                if on_host:   # the host assembly fetches every utterance's transformed features
                    assert syncs[-1] - syncs[0] >= n_utt
                else:         # gathered on the device: no read waits for it
                    assert syncs[-1] == syncs[0]
        for g0, g1 in zip(legs[0], legs[1]):
            assert np.array_equal(bits(g0["feat"].cpu().numpy()), bits(g1["feat"].cpu().numpy()))
            assert np.array_equal(g0["labels"].cpu().numpy(), g1["labels"].cpu().numpy())
            assert np.array_equal(g0["mask"].cpu().numpy(), g1["mask"].cpu().numpy())


def test_label_beyond_the_output_width_is_an_error(aslp, dev, corpus):
    r = aslp.SequenceReader(corpus["feats"], corpus["post"], batch_size=B, num_stream=3)
    with pytest.raises(RuntimeError, match="Out-of-bound Posterior element"):
        for _ in range(50):
            r.Read(num_pdf=A - 6)
