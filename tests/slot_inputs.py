"""The corpus of the grouped-parse tests (CPU and GPU): name -> (text, format,
max_rows, final).  Each text reaches one rule of include/psg.h's "Text ingest
by feature group"."""
import slot_ref as S

A, L = S.ADFEA, S.LIBSVM


def corpus():
    c = {}

    def add(name, text, fmt=A, max_rows=None, final=True):
        c[name] = (text, fmt, max_rows, final)

    add("slot_ids", b"a 1 1 11:1 12:9 13:10 14:255 15:256 16:257 17:4095\n"
                    b"b 1 0 21:4095 22:257 23:1\n")
    add("leading_zero_fast", b"a 1 1 5:07 6:0007\n")
    add("slow_accepted", b"a 1 1 5:00007 6:+7 8:7\n")
    add("tab_slot", b"a 1 1 5:\t7 6:7\n")
    add("wraps_to_1", b"a 1 1 5:4294967297 6:1\n")
    add("slot_0", b"a 1 1 5:1\nb 1 1 5:0\nc 1 1 5:2\n")
    add("slot_4096", b"a 1 1 5:1\nb 1 1 5:4096\nc 1 1 5:2\n")
    add("slot_negative", b"a 1 1 5:1\nb 1 1 5:-1\nc 1 1 5:2\n")
    add("slot_junk", b"a 1 1 5:1\nb 1 1 5:7x\nc 1 1 5:2\n")
    add("slot_cr_then_token", b"a 1 1 5:1\nb 1 1 5:7\r 6:2\nc 1 1 5:2\n")
    add("crlf", b"a 1 1 5:1 6:2\r\nb 1 0 7:3\r\n")
    add("crcrlf", b"a 1 1 5:1\nb 1 0 7:3\r\r\nc 1 1 5:2\n")
    add("lone_cr_line_end", b"a 1 1 5:1 \r\nb 1 0 7:3 \r\n")
    add("final_cr", b"a 1 1 5:1\nb 1 0 7:3\r")
    add("final_cr_not_final", b"a 1 1 5:1\nb 1 0 7:3\r", final=False)
    add("final_no_newline", b"a 1 1 5:1\nb 1 0 7:3")
    add("no_entry", b"id 1 1\nb 1 0 7:3\n")
    add("dangling_key", b"id 1 1 5:2 9\nb 1 0 7:3\n")
    add("dangling_key_final", b"b 1 0 7:3\nid 1 1 5:2 9")
    add("bad_first", b"a 1 x 5:1\nb 1 1 5:1\n")
    add("bad_middle", b"a 1 1 5:1\nb 1 1 5x:1\nc 1 1 5:2\n")
    add("bad_last", b"a 1 1 5:1\nb 1 1 5:1\nc 1\n")
    add("max_rows", b"a 1 1 5:1\nb 1 1 5:2\nc 1 1 5:3\n", max_rows=2)
    add("max_rows_before_bad", b"a 1 1 5:1\nb 1 1 5:0\n", max_rows=1)
    add("label_forms", b"a 1 -3 5:1\nb 1 +1 5:1\nc 1 0 5:1\nd 1 \t2 5:1\n")
    add("key_forms", b"a 1 1 18446744073709551615:1 0:2 +5:3 99999999999999999999999:4\n")
    add("empty_lines", b"\na 1 1 5:1\n")
    add("nul", b"a 1 1 5:1\nb 1 1 \x005:1\n")
    add("mixed_cr", b"a 1 1 5\r:1\n")
    add("empty", b"")
    add("libsvm", b"1 3:1.5 7:2\n-1 2:0.25\r\n0.5\n1 4:1 4:2\n", fmt=L)
    add("libsvm_bad", b"1 3:1.5\n1 7:1 3:2\n1 1:1\n", fmt=L)
    return c
