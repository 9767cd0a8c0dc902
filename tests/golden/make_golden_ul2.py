"""Generate tests/golden/ul2_collator.npz from the IMPORTED reference (build container only).

    python tests/golden/make_golden_ul2.py

Imports /root/reference (read-only) and runs its `DataCollatorForUL2MLM` (src/data/data_collator_ul2.py) with a stub tokenizer,
one example per call (`batch_size == len(examples) == 1`, so the reference packs nothing) and one denoiser per call (one-hot
proportions).  numpy is seeded; `random_spans_noise_mask` is wrapped so that every mask it draws is recorded.  The fixture is DATA
(arrays): raw tokens, lengths, denoiser index, the recorded masks, the reference's input_ids / labels, and its
`denoiser_optimal_len` at two (max_length, max_labels_length) settings.  No reference source text is stored.

Denoisers: the set of the reference's train_flash_t5.py (six span denoisers and the sequential one) with max_spans 100, one with
max_spans = 7, one with an empty prefix.  Lengths: every n from 11 (the reference drops shorter examples) to the denoiser's own
optimum at max_length = 160 -- this crosses the half-to-even cases n * 0.5 with odd n.  Every fifth case holds raw eos tokens.
NO case is skipped silently: a case either compares or is one the reference itself raises on, and those are stored apart
(`raised_*`; the encoder side is one column too long for max_length, which the device collator reports as status bit 1) and
asserted to be exactly the last two lengths of the mu = 64, r = 0.15 denoiser: its optimum counts rint(noise / mu) = 0 sentinels
where the mask has one."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

SENTINEL_FIRST, NUM_SENTINELS, EOS, PAD = 32099, 100, 1, 0
PREFIXES = {"[R]": [31990, 31991], "[S]": [31992], "[X]": [31993, 31994, 31995], "": []}
DENOISERS = [
    {"mu": 3.0, "r": 0.15, "max_spans": 100, "prefix": "[R]"},
    {"mu": 8.0, "r": 0.15, "max_spans": 100, "prefix": "[R]"},
    {"mu": 4.0, "r": 0.0, "max_spans": 1, "prefix": "[S]"},
    {"mu": 3.0, "r": 0.5, "max_spans": 100, "prefix": "[X]"},
    {"mu": 8.0, "r": 0.15, "max_spans": 100, "prefix": "[X]"},
    {"mu": 64.0, "r": 0.15, "max_spans": 100, "prefix": "[X]"},
    {"mu": 64.0, "r": 0.5, "max_spans": 100, "prefix": "[X]"},
    {"mu": 3.0, "r": 0.15, "max_spans": 7, "prefix": "[R]"},
    {"mu": 3.0, "r": 0.5, "max_spans": 100, "prefix": ""},
]
SETTINGS = [(160, 160), (1024, 1024)]
MIN_LEN = 11
TOKEN_VOCAB = 48   # raw tokens are drawn from [2, 50): a small alphabet keeps the compressed fixture to a few hundred KB


class StubTokenizer:
    eos_token_id, pad_token_id = EOS, PAD
    all_special_tokens = ["</s>", "<pad>"] + [f"<extra_id_{i}>" for i in range(NUM_SENTINELS)]
    all_special_ids = [EOS, PAD] + [SENTINEL_FIRST - i for i in range(NUM_SENTINELS)]

    def encode(self, text, return_tensors=None):
        return np.array([PREFIXES[text] + [EOS]], dtype=np.int64)


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_data_collator_ul2", os.path.join(REF, "src", "data", "data_collator_ul2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.DataCollatorForUL2MLM


def main():
    Collator = load_reference()
    D = len(DENOISERS)
    tok = StubTokenizer()
    optimal = np.zeros((len(SETTINGS), D, 2), dtype=np.int32)
    for s, (ml, mll) in enumerate(SETTINGS):
        c = Collator(tok, ml, mll, 1, DENOISERS, [1.0 / D] * D)
        optimal[s] = np.array(c.denoiser_optimal_len, dtype=np.int64)
    ml, mll = SETTINGS[0]
    lmax = int(optimal[0, :, 0].max())
    np.random.seed(20240517)
    rng = np.random.default_rng(7)   # the raw tokens (the reference draws from numpy's global generator)
    rows = dict(tokens=[], lengths=[], denoiser=[], mask=[], ref_input_ids=[], ref_labels=[])
    raised = dict(tokens=[], lengths=[], denoiser=[])
    planned = 0
    for d in range(D):
        onehot = [1.0 if i == d else 0.0 for i in range(D)]
        c = Collator(tok, ml, mll, 1, DENOISERS, onehot)
        masks = []
        inner = c.random_spans_noise_mask
        c.random_spans_noise_mask = lambda n, params, inner=inner, masks=masks: (masks.append(inner(n, params)), masks[-1])[1]
        for n in range(MIN_LEN, int(optimal[0, d, 0]) + 1):
            planned += 1
            t = rng.integers(2, 2 + TOKEN_VOCAB, size=n)
            if planned % 5 == 0:
                t[rng.integers(0, n, size=3)] = EOS
            padded = np.zeros(lmax, dtype=np.int32)
            padded[:n] = t
            del masks[:]
            try:
                batch = c([{"input_ids": t[None, :].astype(np.int64)}])
            except ValueError:
                raised["tokens"].append(padded), raised["lengths"].append(n), raised["denoiser"].append(d)
                continue
            assert len(masks) == 1 and masks[0].shape == (n,)
            m = np.zeros(lmax, dtype=np.uint8)
            m[:n] = masks[0]
            ids, labels = batch["input_ids"].numpy(), batch["labels"].numpy()
            assert ids.shape == (1, ml) and labels.shape == (1, mll)
            rows["tokens"].append(padded), rows["lengths"].append(n), rows["denoiser"].append(d), rows["mask"].append(m)
            rows["ref_input_ids"].append(ids[0].astype(np.int32)), rows["ref_labels"].append(labels[0].astype(np.int32))
    # no case skipped: everything planned either compared or raised, and what raised is the one known case
    assert len(rows["lengths"]) + len(raised["lengths"]) == planned
    for n, d in zip(raised["lengths"], raised["denoiser"]):
        assert (DENOISERS[d]["mu"], DENOISERS[d]["r"]) == (64.0, 0.15) and n >= optimal[0, d, 0] - 1, (n, d)
    assert len(raised["lengths"]) == 2, raised["lengths"]
    off = np.cumsum([0] + [len(PREFIXES[x["prefix"]]) for x in DENOISERS]).astype(np.int32)
    out = os.path.join(HERE, "ul2_collator.npz")
    np.savez_compressed(
        out, tokens=np.stack(rows["tokens"]), lengths=np.array(rows["lengths"], dtype=np.int32),
        denoiser=np.array(rows["denoiser"], dtype=np.int32), mask=np.stack(rows["mask"]),
        ref_input_ids=np.stack(rows["ref_input_ids"]), ref_labels=np.stack(rows["ref_labels"]),
        raised_tokens=np.stack(raised["tokens"]), raised_lengths=np.array(raised["lengths"], dtype=np.int32),
        raised_denoiser=np.array(raised["denoiser"], dtype=np.int32),
        den_mu=np.array([x["mu"] for x in DENOISERS]), den_r=np.array([x["r"] for x in DENOISERS]),
        den_max_spans=np.array([x["max_spans"] for x in DENOISERS], dtype=np.int32), prefix_off=off,
        prefix_ids=np.array([t for x in DENOISERS for t in PREFIXES[x["prefix"]]], dtype=np.int64),
        settings=np.array(SETTINGS, dtype=np.int32), optimal_len=optimal,
        vocab=np.array([SENTINEL_FIRST, NUM_SENTINELS, EOS, PAD], dtype=np.int64))
    print(f"{out}: {len(rows['lengths'])} compared cases, {len(raised['lengths'])} the reference raises on, "
          f"{os.path.getsize(out) / 1024:.0f} KiB; optimal lengths at {SETTINGS[0]}: {optimal[0].tolist()}")


if __name__ == "__main__":
    sys.exit(main())
