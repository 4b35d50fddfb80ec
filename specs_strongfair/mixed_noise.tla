------------------------------ MODULE mixed_noise ------------------------------
(* Written to show: MIXED FAIRNESS: the waiter is `fair+ process`, the flipper `process`, the noise `fair process`.  The waiter awaits turn = 1 (enabled now and then), the flipper flips the turn (enabled always), the noise flips a bit of its own for ever.  Nothing obliges the flipper to move: the noise alone runs, the turn stays 0 and the waiter is never enabled.  <>(got = 1) is VIOLATED.  The three files of this family differ in the keywords only. *)
EXTENDS Naturals

(* --algorithm mixed_noise
variables turn = 0, got = 0, bit = 0;

fair+ process Waiter = 0
begin
  W:   await turn = 1;
  Got: got := 1;
end process

process Flipper = 1
begin
  F: while got = 0 do
       turn := 1 - turn;
     end while;
end process

fair process Noise = 2
begin
  N: while got = 0 do
       bit := 1 - bit;
     end while;
end process

end algorithm *)

Gets == <>(got = 1)
=============================================================================
