"""CPU: the host side of generate.py (the program) and of the generation library behind it - argument parsing, style sampling, the style
file rule, length bucketing and the two writers. No device is touched."""
import os
import pickle
import random

import numpy as np
import pytest


def test_addtoconfig_parsing_nests_and_coerces_like_the_reference():
    """reference generate.py:116-136, 941-946: items split at ',', each item at '=' into keys... and a value; the last key is set on the
    dictionary the earlier keys lead to; int, then float, then text; an empty value is None"""
    import generate as cli
    from handwriting_line_generation_amd.generate import apply_add_to_config
    adds = cli.parse_addtoconfig("model=style_dim=64,trainer=foo=,model=count_std=0.25,name=abc,gpu=3")
    assert adds == [["model", "style_dim", "64"], ["trainer", "foo", ""], ["model", "count_std", "0.25"], ["name", "abc"], ["gpu", "3"]]
    config = {"model": {"style_dim": 128, "other": 1}, "trainer": {"foo": 5}, "name": "x"}
    out = apply_add_to_config(config, adds)
    assert out is config
    assert config == {"model": {"style_dim": 64, "other": 1, "count_std": 0.25}, "trainer": {"foo": None}, "name": "abc", "gpu": 3}
    assert type(config["model"]["style_dim"]) is int and type(config["model"]["count_std"]) is float
    # an item without '=' (an IndexError in the reference) is a key in front of the next item
    assert cli.parse_addtoconfig("model,style_dim=64") == [["model", "style_dim", "64"]]
    assert cli.parse_addtoconfig("trainer,foo=") == [["trainer", "foo", ""]]
    config2 = apply_add_to_config({"model": {"style_dim": 128}, "trainer": {"foo": 5}}, cli.parse_addtoconfig("model,style_dim=64,trainer,foo=,model,count_std=1e-3"))
    assert config2 == {"model": {"style_dim": 64, "count_std": 0.001}, "trainer": {"foo": None}}
    assert type(config2["model"]["style_dim"]) is int and type(config2["model"]["count_std"]) is float
    with pytest.raises(SystemExit):
        cli.parse_addtoconfig("model,style_dim")
    assert cli.parse_addtoconfig(None) == [] and apply_add_to_config({"a": 1}, None) == {"a": 1}
    with pytest.raises(KeyError):
        apply_add_to_config({"model": {}}, [["missing", "k", "1"]])
    with pytest.raises(ValueError):
        apply_add_to_config({"model": {}}, [["model"]])


def test_run_parsing_gives_a_dict():
    import generate as cli
    assert cli.parse_run("choice=R,num=5,text=texts.txt") == {"choice": "R", "num": "5", "text": "texts.txt"}
    assert cli.parse_run("choice=f,path1=a.png,path2=b.png,text=") == {"choice": "f", "path1": "a.png", "path2": "b.png", "text": ""}
    with pytest.raises(SystemExit):
        cli.parse_run("choice")


def test_without_run_the_program_exits_with_the_message(tmp_path):
    import generate as cli
    with pytest.raises(SystemExit) as e:
        cli.main(["-c", str(tmp_path / "none.pth"), "-d", str(tmp_path / "out")])
    assert e.value.code not in (None, 0) and "interactive prompt is not built" in str(e.value.code) and "-r choice=R" in str(e.value.code)
    assert not (tmp_path / "out").exists()


def test_unknown_choice_names_the_two_that_exist(tmp_path):
    import generate as cli
    with pytest.raises(NotImplementedError) as e:
        cli.main(["-c", str(tmp_path / "none.pth"), "-d", str(tmp_path / "out"), "-r", "choice=m"])
    assert "'R'" in str(e.value) and "'f'" in str(e.value) and "'m'" in str(e.value)


def _style_dict():
    g = np.random.RandomState(11)
    return {"a7": [g.randn(8).astype(np.float32) for _ in range(3)], "b2": [g.randn(8).astype(np.float32)],
            "c9": [g.randn(8).astype(np.float32) for _ in range(2)]}


def test_sample_styles_draws_in_the_reference_order():
    """reference generate.py:385-405: choice, randint, choice, randint, random per instance; inter = 2 r - 0.5"""
    from handwriting_line_generation_amd.generate import sample_styles
    styles = _style_dict()
    rand = random.Random(3)
    got = sample_styles(styles, 6, rand)
    ref_rand = random.Random(3)
    want = []
    for _ in range(6):
        author_a = ref_rand.choice(list(styles.keys()))
        s1 = styles[author_a][ref_rand.randint(0, len(styles[author_a]) - 1)]
        author_b = ref_rand.choice(list(styles.keys()))
        s2 = styles[author_b][ref_rand.randint(0, len(styles[author_b]) - 1)]
        inter = 2 * ref_rand.random() - 0.5
        want.append(s1 * inter + s2 * (1 - inter))
    want = np.stack(want)
    assert got.dtype == np.float32 and got.shape == (6, 8)
    assert got.tobytes() == want.astype(np.float32).tobytes()
    assert rand.getstate() == ref_rand.getstate()
    assert len({r.tobytes() for r in got}) > 1


def test_load_style_file_star_rule_merge_and_ids(tmp_path):
    """reference generate.py:215-239: the location is a prefix ('*' appended unless it ends in one), every matching pickle is read and
    merged per author; the `ids` entry is optional"""
    from handwriting_line_generation_amd.evaluate import dump_styles
    from handwriting_line_generation_amd.generate import load_style_file
    g = np.random.RandomState(5)
    s_a, s_b = g.randn(3, 8).astype(np.float32), g.randn(2, 8).astype(np.float32)
    dump_styles({"styles": s_a, "authors": ["w1", "w2", "w1"]}, str(tmp_path / "styles.pkl"))
    with open(str(tmp_path / "styles.pkl.part2"), "wb") as f:         # as get_styles.py writes it, with the ids of the lines behind each style
        pickle.dump({"styles": s_b, "authors": ["w2", "w3"], "ids": [["l1", "l2"], ["l3"]]}, f)
    for loc in (str(tmp_path / "styles.pkl"), str(tmp_path / "styles.pkl*"), str(tmp_path / "styles")):
        got = load_style_file(loc)
        assert list(got.keys()) == ["w1", "w2", "w3"]
        assert [len(v) for v in got.values()] == [2, 2, 1]
        assert np.array_equal(got["w1"][0], s_a[0]) and np.array_equal(got["w1"][1], s_a[2])
        assert np.array_equal(got["w2"][0], s_a[1]) and np.array_equal(got["w2"][1], s_b[0]) and np.array_equal(got["w3"][0], s_b[1])
    only = load_style_file(str(tmp_path / "styles.pkl.part"))
    assert list(only.keys()) == ["w2", "w3"]
    with pytest.raises(FileNotFoundError):
        load_style_file(str(tmp_path / "nothing_here"))


def test_length_bucketing():
    from handwriting_line_generation_amd.generate import bucket_by_length
    from handwriting_line_generation_amd.utils.string_utils import str2label_single
    char_to_idx = {c: i + 1 for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")}
    texts = ["hello", "hi", "wor#ld", "##", "no", "ok", "abc", "", "a b", "zz", "x#y", "q!"]
    batches, skipped = bucket_by_length(texts, char_to_idx, batch_lines=3)
    assert skipped == [3, 7]                                   # "##" and "" encode to no label
    seen = [i for _, idx in batches for i in idx]
    assert sorted(seen) == [i for i in range(len(texts)) if i not in skipped] and len(set(seen)) == len(seen)
    for n, idx in batches:
        assert 1 <= len(idx) <= 3
        assert all(len(str2label_single(texts[i], char_to_idx)) == n for i in idx)      # characters outside the set dropped before the count
    assert [n for n, _ in batches] == [5, 2, 2, 3, 1]          # "wor#ld" is 5 labels, "x#y" 2, "q!" 1; 5 lines of 2 labels -> 3 + 2
    assert dict((tuple(idx), n) for n, idx in batches)[(0, 2)] == 5
    one, _ = bucket_by_length(texts, char_to_idx, batch_lines=1)
    assert all(len(idx) == 1 for _, idx in one) and len(one) == 10
    with pytest.raises(ValueError):
        bucket_by_length(texts, char_to_idx, batch_lines=0)


def test_line_widths_rule():
    """4 * (T - round(padded * T)) with T = image width / 4, clamped to [4, image width]"""
    from handwriting_line_generation_amd.generate import line_widths
    T = 37
    padded = [(T - n) / T for n in (37, 36, 1, 0, 20)]
    assert line_widths(padded, 4 * T) == [148, 144, 4, 4, 80]
    assert line_widths([-0.1, 1.2], 40) == [40, 4]


def _ragged_lines():
    g = np.random.RandomState(2)
    return [g.randint(0, 256, (64, w)).astype(np.uint8) for w in (4, 40, 12, 1028, 36)]


def test_shard_writer_round_trips_ragged_lines(tmp_path):
    import generate as cli
    lines, index = _ragged_lines(), [7, 0, 3, 2, 9]
    cli.write_shard(str(tmp_path / "one.npz"), lines, index)
    with np.load(str(tmp_path / "one.npz")) as z:
        assert z["pixels"].dtype == np.uint8 and z["pixels"].ndim == 1 and z["pixels"].size == 64 * sum(l.shape[1] for l in lines)
        assert z["offsets"].dtype == np.int64 and z["offsets"].tolist() == [0] + np.cumsum([l.size for l in lines]).tolist()
        assert z["widths"].dtype == np.int32 and z["widths"].tolist() == [l.shape[1] for l in lines]
        assert z["index"].dtype == np.int64 and z["index"].tolist() == index
    back = cli.read_shard(str(tmp_path / "one.npz"))
    assert [i for i, _ in back] == index and all(np.array_equal(a, b) for (_, a), b in zip(back, lines))
    # through the sink: 5 lines in shards of 2 -> 2 + 2 + 1
    sink = cli.LineSink(str(tmp_path), "sample_%d.png", shard=2, writers=3)
    for i, l in zip(index, lines):
        sink.add(i, l)
    sink.close()
    names = sorted(n for n in os.listdir(str(tmp_path)) if n.startswith("lines_"))
    assert names == ["lines_00000.npz", "lines_00001.npz", "lines_00002.npz"]
    got = [p for n in names for p in cli.read_shard(str(tmp_path / n))]
    assert [i for i, _ in got] == index and all(np.array_equal(a, b) for (_, a), b in zip(got, lines))


def test_png_writer_round_trips_ragged_lines(tmp_path):
    from PIL import Image
    import generate as cli
    lines, index = _ragged_lines(), [7, 0, 3, 2, 9]
    sink = cli.LineSink(str(tmp_path), "sample_%d.png", shard=0, writers=100)
    assert sink.pool._max_workers == cli.MAX_WRITERS == 16          # never more than 16 encoder threads, whatever is asked for
    for i, l in zip(index, lines):
        sink.add(i, l)
    sink.close()
    assert sorted(os.listdir(str(tmp_path))) == sorted("sample_%d.png" % i for i in index)
    for i, l in zip(index, lines):
        im = Image.open(str(tmp_path / ("sample_%d.png" % i)))
        assert im.mode == "L" and im.size == (l.shape[1], 64) and np.array_equal(np.asarray(im), l)


def test_lines_to_u8_entry_point_refuses_bad_arguments_before_any_launch():
    """the argument checks of hwg_lines_to_u8 run on the host side of the entry point, in front of the launch: with arguments they refuse,
    the call returns its status without a device (the addresses are never dereferenced)"""
    from handwriting_line_generation_amd import _lib as L
    p = 1 << 20          # any 16-byte aligned address
    for args, word in [((p, 1, 64, 42, p, p, p, 0), "multiple of 4"), ((p, 0, 64, 44, p, p, p, 0), "bad sizes"),
                       ((p, 1, 0, 44, p, p, p, 0), "bad sizes"), ((p, 70000, 64, 44, p, p, p, 0), "bad sizes"),
                       ((None, 1, 64, 44, p, p, p, 0), "null"), ((p, 1, 64, 44, None, p, p, 0), "null"),
                       ((p, 1, 64, 44, p, None, p, 0), "null"), ((p, 1, 64, 44, p, p, None, 0), "null"),
                       ((p + 4, 1, 64, 44, p, p, p, 0), "aligned"), ((p, 1, 64, 44, p, p, p + 2, 0), "aligned")]:
        with pytest.raises(L.HwgError) as e:
            L.call("hwg_lines_to_u8", *args)
        assert word in str(e.value), (args, str(e.value))
