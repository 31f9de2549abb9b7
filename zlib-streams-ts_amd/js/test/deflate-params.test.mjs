// windowBits and memLevel through the JavaScript host path (streams-api.mjs -> zsnapi.node
// -> zs_pool_deflate_batch_params): compressBatch*(inputs, format, {level, windowBits, memLevel}),
// goldens of tests/golden/deflate_params.json (C zlib 1.2.11), the outputs read back through
// node's own zlib, and the rejection rules.
//   node deflate-params.test.mjs cpu   -- the argument checks only (no GPU needed)
import crypto from "crypto";
import fs from "fs";
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;
const digest = (b) => [b.length, crypto.createHash("sha256").update(b).digest("hex").slice(0, 16)];

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

async function argumentChecks() {
  const one = [new Uint8Array([1, 2, 3])];
  const dict = new Uint8Array([1, 2, 3, 4]);
  // deflateInit2_'s Z_STREAM_ERROR (deflate.ts:281-294), refused before any device is touched
  const bad = [["deflate", { windowBits: 7 }], ["deflate", { windowBits: 16 }], ["deflate-raw", { windowBits: 8 }],
               ["gzip", { windowBits: 8 }], ["deflate", { windowBits: 12.5 }], ["deflate", { memLevel: 0 }],
               ["deflate", { memLevel: 10 }], ["gzip", { windowBits: 12, memLevel: -1 }]];
  for (const [format, options] of bad) {
    const what = format + " " + JSON.stringify(options);
    await rejects(api.compressBatch(one, format, options), (e) => e.message === "init failed: -2", what);
    await rejects(api.compressBatchSettled(one, format, options), (e) => e.message === "init failed: -2", "settled: " + what);
    await rejects(api.compressBatchDetailed(one, format, options), (e) => e.code === "-2", "detailed: code -2: " + what);
  }
  for (const options of [{ windowBits: 12 }, { memLevel: 4 }, { windowBits: 9, memLevel: 1 }]) {
    await rejects(api.compressBatch(one, "deflate-raw", { ...options, dictionary: dict }), (e) => e instanceof TypeError,
                  "with a dictionary: a TypeError");
    await rejects(api.compressBatch(one, "deflate", { ...options, strategy: api.Z_FIXED }), (e) => e instanceof TypeError,
                  "with a strategy: a TypeError");
    await rejects(api.compressBatchDetailed(one, "deflate", { ...options, dictionary: [dict] }), (e) => e instanceof TypeError,
                  "the detailed entry checks it too");
  }
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const golden = JSON.parse(fs.readFileSync(new URL("../../../tests/golden/deflate_params.json", import.meta.url)));
  const text = (k, n) => corpus.text(corpus.streamSeed(k), n);
  // [golden, input, format, level, windowBits, memLevel] -- the inputs of tests/paramcases.py
  const cases = [
    ["hash/deflate-raw/l6/w15/m9/T8192", text(5000, 8192), "deflate-raw", 6, 15, 9],
    ["hash/deflate-raw/l1/w15/m9/T8192", text(5000, 8192), "deflate-raw", 1, 15, 9],
    ["hash/deflate/l1/w10/m3/T8192", text(5000, 8192), "deflate", 1, 10, 3],
    ["slide/deflate-raw/l6/w9/m8/T762", text(5201, 762), "deflate-raw", 6, 9, 8],
    ["long/deflate-raw/l6/w12/m4/T200000", text(5401, 200000), "deflate-raw", 6, 12, 4],
    ["tiny/gzip/l6/w9/m8/n3", new Uint8Array([97, 98, 99]), "gzip", 6, 9, 8],
    ["tiny/deflate/l6/w8/m8/n3", new Uint8Array([97, 98, 99]), "deflate", 6, 8, 8],
  ];
  const inflate = { "deflate-raw": zlib.inflateRawSync, deflate: zlib.inflateSync, gzip: zlib.gunzipSync };
  for (const [name, x, format, level, windowBits, memLevel] of cases) {
    expect(golden[name] !== undefined, "golden " + name);
    const options = { level, windowBits, memLevel };
    const inputs = [x, new Uint8Array(0), x.subarray(0, x.length >> 1), x];
    const outs = await api.compressBatch(inputs, format, options);
    expect(JSON.stringify(digest(outs[0])) === JSON.stringify(golden[name]), name + ": zlib 1.2.11's bytes");
    expect(same(outs[0], outs[3]), name + ": the same input twice");
    outs.forEach((o, i) => expect(same(new Uint8Array(inflate[format](o)), inputs[i]), `${name}: node's zlib, input ${i}`));
    const back = await api.decompressBatch(outs, format);
    back.forEach((o, i) => expect(same(o, inputs[i]), `${name}: the engine's inflate, input ${i}`));
    const det = await api.compressBatchDetailed(inputs, format, options);
    det.outputs.forEach((o, i) => expect(det.status[i] === 1 && same(o, outs[i]), `${name}: detailed, input ${i}`));
    const settled = await api.compressBatchSettled(inputs, format, options);
    settled.forEach((s, i) => expect(s.status === "fulfilled" && same(s.value, outs[i]), `${name}: settled, input ${i}`));
  }
  // values that are not numbers mean 15 / 8, and 15 / 8 is the plain call -- also with a dictionary or a strategy
  const x = text(5000, 8192);
  const plain = await api.compressBatch([x], "deflate", { level: 6 });
  for (const v of [undefined, null, "12", {}])
    expect(same((await api.compressBatch([x], "deflate", { level: 6, windowBits: v, memLevel: v }))[0], plain[0]),
           "windowBits / memLevel " + String(v) + " are the defaults");
  expect(same((await api.compressBatch([x], "deflate", { level: 6, windowBits: 15, memLevel: 8 }))[0], plain[0]), "15 / 8 is the plain call");
  expect(!same((await api.compressBatch([x], "deflate", { level: 6, windowBits: 12 }))[0], plain[0]), "windowBits 12 is not");
  const fixed = await api.compressBatch([x], "deflate", { level: 6, strategy: api.Z_FIXED });
  expect(same((await api.compressBatch([x], "deflate", { level: 6, strategy: api.Z_FIXED, windowBits: 15, memLevel: 8 }))[0], fixed[0]),
         "15 / 8 with a strategy");
  // level 0 with other parameters is not built; an invalid level fails as without them
  await rejects(api.compressBatch([x], "deflate", { level: 0, windowBits: 12 }), (e) => e.message === "init failed: -2", "level 0");
  await rejects(api.compressBatch([x], "deflate", { level: 10, memLevel: 4 }), (e) => e.message === "init failed: -2", "level 10");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e); process.exit(1); });
