// The BGZF writer through the JavaScript host path (streams-api.mjs -> zsnapi.node ->
// zs_pool_deflate_batch_bgzf): compressBatch*(inputs, "gzip", {level, bgzf: true | blockBytes}), goldens of
// tests/golden/deflate_bgzf.json (C zlib 1.2.11 in the framing of include/zs_gpu.h), the outputs read back
// through node's own zlib and the engine's {members: "bgzf"}, and the rejection rules.
//   node deflate-bgzf.test.mjs cpu   -- the argument checks only (no GPU needed)
import crypto from "crypto";
import fs from "fs";
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;
const digest = (b) => [b.length, crypto.createHash("sha256").update(b).digest("hex").slice(0, 16)];
const EOF = new Uint8Array(Buffer.from("1f8b08040000000000ff0600424302001b0003000000000000000000", "hex"));

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

async function argumentChecks() {
  const one = [new Uint8Array([1, 2, 3])];
  const dict = new Uint8Array([1, 2, 3, 4]);
  const type = (e) => e instanceof TypeError;
  expect(api.BGZF_BLOCK === 65280, "BGZF_BLOCK");
  // a gzip notion, and not built together with the other features: refused before any device is touched
  for (const bgzf of [true, 4096]) {
    await rejects(api.compressBatch(one, "deflate", { bgzf }), type, "format deflate: a TypeError");
    await rejects(api.compressBatch(one, "deflate-raw", { bgzf }), type, "format deflate-raw: a TypeError");
    await rejects(api.compressBatch(one, "gzip", { bgzf, strategy: api.Z_FIXED }), type, "with a strategy: a TypeError");
    await rejects(api.compressBatch(one, "gzip", { bgzf, windowBits: 12 }), type, "with windowBits: a TypeError");
    await rejects(api.compressBatchSettled(one, "gzip", { bgzf, memLevel: 4 }), type, "with memLevel: a TypeError");
    await rejects(api.compressBatch(one, "gzip", { bgzf, flushAt: [1] }), type, "with flushAt: a TypeError");
    await rejects(api.compressBatch(one, "gzip", { bgzf, flushEvery: 2 }), type, "with flushEvery: a TypeError");
    await rejects(api.compressBatchDetailed(one, "gzip", { bgzf, dictionary: [dict] }), type, "with a dictionary: a TypeError");
  }
  for (const bgzf of [0, -1, 1.5, "64k", {}])
    await rejects(api.compressBatch(one, "gzip", { bgzf }), type, JSON.stringify(bgzf) + ": a TypeError");
  // the addon's own checks, before any device is touched: code "-2"
  await rejects(api.compressBatchDetailed(one, "gzip", { bgzf: 65281 }), (e) => e.code === "-2", "a block size above 65,280");
  await rejects(api.compressBatch(one, "gzip", { bgzf: 65281 }), (e) => e.message === "init failed: -2", "... as the init error");
}

// the members of a BGZF file read from their headers: [[offset, BSIZE + 1, ISIZE]]
function members(file) {
  const out = [];
  const dv = new DataView(file.buffer, file.byteOffset, file.length);
  for (let p = 0; p < file.length;) {
    expect(dv.getUint32(p, false) === 0x1f8b0804 && dv.getUint16(p + 10, true) === 6 && file[p + 12] === 66 && file[p + 13] === 67,
           "a BGZF header at " + p);
    expect(file[p + 8] === 0 && file[p + 9] === 255, "XFL 0, OS 255 at " + p);
    const size = dv.getUint16(p + 16, true) + 1;
    out.push([p, size, dv.getUint32(p + size - 4, true)]);
    p += size;
  }
  return out;
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const golden = JSON.parse(fs.readFileSync(new URL("../../../tests/golden/deflate_bgzf.json", import.meta.url)));
  const text = (k, n) => corpus.text(corpus.streamSeed(k), n);
  const B = 65280;
  const edge = text(7000, 2 * B + 1);
  // [golden, input, level, bgzf] -- the inputs of tests/bgzfwritecases.py
  const cases = [
    ["empty/l6/b65280/empty", new Uint8Array(0), 6, true],
    ["edge/l6/b65280/T1", edge.subarray(0, 1), 6, true],
    ["edge/l1/b65280/T65281", edge.subarray(0, B + 1), 1, true],
    ["edge/l9/b65280/T130561", edge, 9, B],
    ["phases/l6/b1/T300", text(7001, 300), 6, 1],
    ["phases/l1/b7/T1000", text(7002, 1000), 1, 7],
    ["many/l6/b256/T153600", text(7200, 153600), 6, 256],
    ["level0/l0/b65280/T65281", text(7400, B + 1), 0, true],
  ];
  for (const [name, x, level, bgzf] of cases) {
    expect(golden[name] !== undefined, "golden " + name);
    const bb = bgzf === true ? B : bgzf;
    const inputs = [x, new Uint8Array(0), x];
    const outs = await api.compressBatch(inputs, "gzip", { level, bgzf });
    expect(JSON.stringify(digest(outs[0])) === JSON.stringify(golden[name]), name + ": the golden's bytes");
    expect(same(outs[0], outs[2]), name + ": the same input twice");
    expect(same(outs[1], EOF), name + ": an empty input is the end-of-file block");
    const ms = members(outs[0]);
    expect(ms.length === Math.ceil(x.length / bb) + 1 && ms[ms.length - 1][1] === 28 && ms[ms.length - 1][2] === 0, name + ": blocks + the end-of-file block");
    expect(ms.slice(0, -1).every((m, i) => m[2] === Math.min(bb, x.length - i * bb)), name + ": ISIZE is the piece's length");
    outs.forEach((o, i) => expect(same(new Uint8Array(zlib.gunzipSync(o)), inputs[i]), `${name}: node's zlib, input ${i}`));
    const back = await api.decompressBatch(outs, "gzip", { members: "bgzf" });
    back.forEach((o, i) => expect(same(o, inputs[i]), `${name}: the engine's BGZF reader, input ${i}`));
    const det = await api.compressBatchDetailed(inputs, "gzip", { level, bgzf });
    det.outputs.forEach((o, i) => expect(det.status[i] === 1 && same(o, outs[i]), `${name}: detailed, input ${i}`));
    expect(det.check[0] === (zlib.crc32 ? zlib.crc32(x) : det.check[2]) && det.check[1] === 0, name + ": the check value is the crc32 of the whole input");
    const settled = await api.compressBatchSettled(inputs, "gzip", { level, bgzf });
    settled.forEach((s, i) => expect(s.status === "fulfilled" && same(s.value, outs[i]), `${name}: settled, input ${i}`));
  }
  await rejects(api.compressBatch([edge], "gzip", { level: 10, bgzf: true }), (e) => e.message === "init failed: -2", "level 10");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e); process.exit(1); });
