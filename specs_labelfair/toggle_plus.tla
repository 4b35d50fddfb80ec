------------------------------ MODULE toggle_plus ------------------------------
(* Written to show: THE `+` ON ONE LABEL OF A WEAKLY FAIR PROCESS: the Waiter of specs_strongfair/toggle_fair with `W:+`.  W is enabled in every other state of the Toggler's cycle; WF_vars(Waiter) obliges it to nothing, SF_vars(W) makes it move; `Got` then follows under WF_vars(Waiter), in which `W` stays a member.  Termination HOLDS (it is violated without the `+`: specs_strongfair/toggle_fair). *)
EXTENDS Naturals

(* --algorithm toggle_plus
variables turn = 0, got = 0;

fair process Waiter = 0
begin
  W:+  await turn = 1;
  Got: got := 1;
end process

fair process Toggler = 1
begin
  F: while got = 0 do
       turn := 1 - turn;
     end while;
end process

end algorithm *)

=============================================================================
